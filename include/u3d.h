/*
 * u3d.h -- C ABI of the MI355X (gfx950) kernels behind UniDet3D's detection hot path.
 *
 * Every entry point replaces an operator the reference reaches through a third-party
 * CUDA package (call sites cited per function, file:line relative to the reference repo).
 * Conventions:
 *   - plain pointers + sizes, no torch types; all pointers are DEVICE pointers unless
 *     the name ends in _host;
 *   - returns 0 on success, a negative U3D_E* code otherwise; never throws;
 *   - the caller owns every buffer; scratch is passed explicitly (`ws`, sized by the
 *     matching *_ws_bytes() query); no hidden allocation, no device synchronisation:
 *     work is enqueued on `stream`; counts the host needs (voxel counts) are read back
 *     by the caller from the documented device words;
 *   - thread-safe for distinct streams.
 * Rows of feature matrices are contiguous fp32 ([N, C] row-major, C % 16 == 0 for the
 * convolution operands).  Voxel rows are in CANONICAL order: ascending
 * key = ((b*X + x)*Y + y)*Z + z.  Rulebook pair lists are grouped by kernel offset and
 * ascending in both columns inside an offset.
 */
#ifndef U3D_H_
#define U3D_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* u3d_stream_t; /* hipStream_t */

#define U3D_OK 0
#define U3D_EINVAL (-1)   /* bad argument / unsupported size */
#define U3D_ELAUNCH (-2)  /* HIP launch error (hipGetLastError != success) */
#define U3D_EUNSUPPORTED (-3) /* channel combination not instantiated */

/* Bumped with every change of an entry point's argument list; unidet3d_amd/_lib.py refuses a library whose version differs from
 * the one it was written against (a stale .so would misread shifted arguments instead of failing).  Entry points that are only
 * ADDED (R15) leave it alone: no existing argument list moves, and _lib.py refuses a library that lacks a declared symbol. */
#define U3D_ABI_VERSION 117
int u3d_version(void);
const char* u3d_last_error(void);
/* How the fp32 matrix kernels (decoder GEMMs, attention, sparse convolutions without U3D_BF16_OPERANDS) multiply:
 *   1 (default; env U3D_FP32_MATH=bf16x3): each fp32 operand is split exactly into three bf16 pieces and a product is six
 *     bf16 MFMAs with fp32 accumulation -- fp32-level error (the dropped terms are below 2^-23 of a product), 2.7x less matrix
 *     pipe time than
 *   0 (env U3D_FP32_MATH=mfma): the native v_mfma_f32_* instructions.
 * Returns the previous mode; any other argument only queries.  Process-wide, not thread-safe against running launches. */
int u3d_fp32_math(int mode);

/* Which output-stationary sparse-convolution kernel serves u3d_spconv_gmm_bf16 / _x3:
 *   1 (default; env U3D_GMM_WG unset or != 0): workgroup tiles -- four waves share 4 x tile_rows dst rows, the packed weights of
 *     an offset are staged once per workgroup in LDS and the offset's pairs are dealt evenly to the waves (csrc/spconv_wg.hip) --
 *     where they measured ahead: the three-plane entry point at k_groups = 1; 2: wherever that kernel is instantiated (tests, A/B);
 *   0: wave-private tiles, every item reads its weight fragments through the vector-memory path (csrc/spconv.hip; also what
 *     u3d_spconv_gmm -- native fp32 MFMAs -- and launches with bn_partial always use).
 * Same arguments, same tile_starts, bit-identical pair arithmetic; results differ only in fp32 summation order across offsets
 * of one row (none: both accumulate offsets in ascending order).  Returns the previous mode; other arguments only query. */
int u3d_conv_kernel(int mode);

/* How many waves of 16 query rows (dK / dV: key rows) share a workgroup of the plane attention kernels (csrc/attn_x3.hip) and with
 * it every staged 64-row K / V (Q / dO) tile:
 *   0 (default; env U3D_ATTN_TILE_WAVES unset or neither 4 nor 8): the launch plan -- per kernel, data flow, head dim and dropout the
 *     form that measured fastest (DESIGN 4.2 "tile waves");
 *   4 | 8: that form for the three kernels of every call (tests, A/B runs).
 * A wave runs the same program in every form: results are bit-identical.  Returns the previous value; other arguments -- 6 among
 * them: a six-wave form was built, measured slower everywhere and removed -- only query. */
int u3d_attn_tile_waves(int waves);

/* ---- kernel timing (HIP events on the launch stream; used by bench.py's roofline) ---- */
enum { U3D_K_CONV_FWD = 0, U3D_K_CONV_WGRAD = 1, U3D_K_BN = 2, U3D_K_POOL = 3, U3D_K_ATTN_FWD = 4,
       U3D_K_ATTN_BWD = 5, U3D_K_RULEBOOK = 6, U3D_K_VOXELIZE = 7, U3D_K_GEMM = 8, U3D_K_COUNT = 9 };
int u3d_prof_enable(int kernel_class, int on);           /* record start/stop events around each launch of the class */
int u3d_prof_collect(int kernel_class, double* total_ms, int64_t* launches, double* work); /* syncs the events, then resets */

/* =====================================================================================
 * R1  voxelisation -- replaces ME.utils.batch_sparse_collate + ME.TensorField(...).sparse()
 *     + field.inverse_mapping (unidet3d/unidet3d.py:158-174).
 * ===================================================================================== */
/* Per-scene min/max of the coordinate source and mean of xyz; also the batch-wide maximum
 * cell index per axis.  points [n_pts, 6] (xyz rgb); coord_src == NULL -> xyz of `points`
 * scaled by 1/voxel_size (unidet3d.py:159), else coord_src [n_pts,3] already in voxel units
 * (elastic path, :164, pass voxel_size = 1).  pt_offsets int64 [B+1].
 * div_mode 0: IEEE divide (what torch's CPU kernel does -- the oracle); 1: multiply by the
 * fp32 reciprocal (what torch's CUDA div-by-scalar kernel does).
 * stats float [B,12] = min[3] max[3] mean_xyz[3] pad[3]; grid_max int32[3]. */
int u3d_vox_scene_stats(const float* points, const float* coord_src, const int64_t* pt_offsets, int B,
                        int64_t max_pts_per_scene, float voxel_size, int div_mode, float* stats,
                        int32_t* grid_max, void* ws, u3d_stream_t stream);
int64_t u3d_vox_scene_stats_ws_bytes(int B);

/* Occupancy index of one level: bitmap uint64 [B*X*Y*Zw] (Zw = ceil(Z/64); bit z&63 of word
 * ((b*X+x)*Y+y)*Zw + (z>>6)) and word_rank int32 [n_words+1] = exclusive popcount prefix, so
 * row(b,x,y,z) = word_rank[w] + popc(bitmap[w] & ((1<<bit)-1)) IS the canonical row.
 * This is a direct-address (perfect-hash) table over the grid EXTENT -- north_star's "hash-built rulebook" with the hash replaced
 * by the cell address, which is what makes the rows come out in canonical order without a sort.  Its size does not depend on
 * occupancy: 12 bytes per 64 z-cells; large extents use the hashed form further down.  u3d_index_words returns the word count, or a negative code when the grid is invalid or
 * would need more than U3D_INDEX_MAX_WORDS words (refused, never allocated). */
#define U3D_INDEX_MAX_WORDS (1LL << 31)
int64_t u3d_index_words(int B, int X, int Y, int Z);
/* sets the bit of every point's cell; writes pt_cell int64 [n_pts] = word*64 + bit (the cell id).  bitmap must be zeroed; bitmap ==
 * NULL: only the cell ids are written (hashed index, below). */
int u3d_vox_mark(const float* points, const float* coord_src, const int64_t* pt_offsets, int B,
                 int64_t max_pts_per_scene, const float* stats, float voxel_size, int div_mode, int X, int Y,
                 int Z, uint64_t* bitmap, int64_t* pt_cell, u3d_stream_t stream);
/* word_rank[0..n_words] ; word_rank[n_words] = number of active voxels (host reads it back). */
int u3d_index_rank(const uint64_t* bitmap, int64_t n_words, int32_t* word_rank, void* ws, u3d_stream_t stream);
int64_t u3d_index_rank_ws_bytes(int64_t n_words);
/* coords int32 [n_vox,4] (b,x,y,z) in canonical order from the index. */
int u3d_index_coords(const uint64_t* bitmap, const int32_t* word_rank, int B, int X, int Y, int Z,
                     int32_t* coords, u3d_stream_t stream);
/* inverse int64 [n_pts] (point -> voxel row); CSR of points per voxel (vox_offsets int32 [n_vox+1],
 * vox_points int32 [n_pts]); feats [n_vox,6] = unweighted mean of [rgb, xyz - mean_xyz(scene)]. */
int u3d_vox_finalize(const float* points, const int64_t* pt_offsets, int B, int64_t n_pts, const float* stats,
                     const int64_t* pt_cell, const uint64_t* bitmap, const int32_t* word_rank, int64_t hash_slots /* 0: bitmap index */, int64_t n_vox,
                     int64_t* inverse, int32_t* vox_offsets, int32_t* vox_points, float* feats, int feat_ld,
                     void* ws, u3d_stream_t stream);
int64_t u3d_vox_finalize_ws_bytes(int64_t n_pts, int64_t n_vox);

/* Hashed form of the index ("hash-built rulebook in HBM", csrc/hashidx.hip) for grids whose extent makes the direct-address
 * table impractical: memory follows OCCUPANCY.  Same contract (cell -> canonical row, rows ascending in the cell id):
 *   u3d_hash_index_build: cells int64 [n] (cell ids as u3d_vox_mark / u3d_cells_of_coords write them; duplicates allowed; entries
 *     equal to INT64_MAX are ignored) -> radix sort (csrc/radix.hip: hand-written stable LSD sort, no library) -> unique: ukeys
 *     int64 [n] (the first *n_unique entries = the occupied cells in canonical order), n_unique device int32 (host reads it back,
 *     like word_rank[n_words]) -> open-addressing table table_keys uint64 [slots] / table_vals int32 [slots] by 64-bit atomicCAS
 *     insertion, slots = u3d_hash_index_slots(n) (power of two >= 2 n).  n_cells: every valid cell id is < n_cells (the grid's
 *     B X Y ceil(Z/64) 64) -- the sort then only runs over the bits the grid needs; 0 = unknown (63 bits).
 *   u3d_hash_index_coords: coords int32 [n,4] of the occupied cells; u3d_cells_of_coords: the (parent) cell of every voxel of a
 *     level (shift = 1: next coarser level, parents outside the halved grid -> INT64_MAX).
 * Every entry point that takes (bitmap, word_rank) also takes `hash_slots`: 0 = bitmap form; > 0 = the two pointers are
 * (table_keys, table_vals) of a table with that many slots.  The rulebook / voxel kernels are the same for both forms. */
int64_t u3d_hash_index_slots(int64_t n);
int64_t u3d_hash_index_ws_bytes(int64_t n);
int u3d_hash_index_build(const int64_t* cells, int64_t n, int64_t n_cells, int64_t* ukeys, int32_t* n_unique, uint64_t* table_keys,
                         int32_t* table_vals, int64_t slots, void* ws, u3d_stream_t stream);
/* The sort itself (keys only, or keys + permutation): keys_in uint64 [n] -> keys_out [n] ascending, STABLE; perm_out (nullable)
 * int32 [n] = position in keys_in of every sorted key.  key_bits: number of significant low bits (passes = ceil(key_bits / 8)).
 * keys_out must not alias keys_in.  Deterministic: no global atomics, ranks by wave ballots in index order. */
int u3d_sort_u64(const uint64_t* keys_in, int64_t n, int key_bits, uint64_t* keys_out, int32_t* perm_out, void* ws, u3d_stream_t stream);
int64_t u3d_sort_ws_bytes(int64_t n, int with_values);
int u3d_hash_index_coords(const int64_t* ukeys, int64_t n, int X, int Y, int Z, int32_t* coords, u3d_stream_t stream);
int u3d_cells_of_coords(const int32_t* coords, int64_t n, int shift, int B, int X2, int Y2, int Z2, int64_t* cells, u3d_stream_t stream);

/* =====================================================================================
 * R2  SubMConv3d rulebook (spconv indice pairs, k=3) -- first conv of each indice_key
 *     subm1..5 (unidet3d/unidet3d.py:97-103, unidet3d/spconv_unet.py:43-56,138).
 *     pair_in/pair_out int32 [27, n]; counts int32 [27]; offset k=(dx+1)*9+(dy+1)*3+(dz+1),
 *     input = output + (dx,dy,dz).
 * ===================================================================================== */
int u3d_subm_rulebook(const int32_t* coords, int64_t n, const uint64_t* bitmap, const int32_t* word_rank, int64_t hash_slots,
                      int B, int X, int Y, int Z, int32_t* pair_in, int32_t* pair_out, int32_t* counts,
                      void* ws, u3d_stream_t stream);
int64_t u3d_subm_rulebook_ws_bytes(int64_t n);

/* =====================================================================================
 * R3  SparseConv3d(k=2,s=2) rulebook, reused by SparseInverseConv3d
 *     (unidet3d/spconv_unet.py:148-154,178-183).  out = in>>1, k=(x&1)*4+(y&1)*2+(z&1),
 *     out dims = floor(in/2), inputs whose parent is out of range are dropped.
 * ===================================================================================== */
/* sets the bit of (b, x>>shift, y>>shift, z>>shift) for every row whose shifted cell is inside (X,Y,Z);
 * shift = 1 builds the next (coarser) level, shift = 0 indexes a caller-supplied coordinate list. bitmap must be zeroed. */
int u3d_index_mark(const int32_t* coords, int64_t n, int shift, int X, int Y, int Z, uint64_t* bitmap,
                   u3d_stream_t stream);
int u3d_down_rulebook(const int32_t* coords, int64_t n, const uint64_t* bitmap2, const int32_t* word_rank2, int64_t hash_slots,
                      int B, int X2, int Y2, int Z2, int32_t* pair_in, int32_t* pair_out, int32_t* counts,
                      void* ws, u3d_stream_t stream);
int64_t u3d_down_rulebook_ws_bytes(int64_t n);

/* =====================================================================================
 * R3g  General convolution geometry: kernel extents 1..3 per axis, any stride, padding, dilation (spconv's SparseConv3d / SubMConv3d
 *      outside the two shapes above).  geom = int32 [12] on the HOST: kernel[3], stride[3], padding[3], dilation[3], axes in the order
 *      of coords[:, 1:4].  Per axis out_dim = floor((in_dim + 2 p - d (k - 1) - 1) / s) + 1; output cell o is active iff an active input
 *      i and a tap t in [0, k) satisfy i + p = o s + t d on all three axes with 0 <= o < out_dim.  Offset index = (t0 k1 + t1) k2 + t2
 *      (the weight layout [C_out, k0, k1, k2, C_in]); K = k0 k1 k2 <= 27.  (k=2, s=2, p=0) gives R3's lists, SubM k=3 (p=1) R2's.
 *   u3d_conv_out_shape (host only): out_shape int32 [3] for input extents (X, Y, Z); an extent that comes out <= 0 is reported as 0.
 *   u3d_conv_mark: the output occupancy of the n input rows `coords`, in one of two forms -- bitmap_out (zeroed, sized by
 *     u3d_index_words(B, out_shape); u3d_index_rank follows) or cells_out int64 [K n] (cell ids, INT64_MAX = none, for
 *     u3d_hash_index_build); exactly one of the two is non-NULL.  The output level's rows are the index's canonical order.
 *   u3d_conv_rulebook: output-stationary pairs.  out_coords int32 [n_out,4] = the output level's rows; (bitmap_in, word_rank_in,
 *     hash_slots, B, X, Y, Z) = the INPUT level's index (n_in rows).  pair_in / pair_out int32 [K, cap], counts int32 [K]; cap >=
 *     min(n_in, n_out) -- enough, because for a fixed offset the map output cell -> input cell is injective and monotone in canonical
 *     order; for the same reason BOTH columns ascend inside an offset and no row repeats, which is what the convolution kernels need.
 *     ws: u3d_conv_rulebook_ws_bytes(n_out, K).
 *   Errors, before any launch and with a u3d_last_error text: U3D_EUNSUPPORTED for a kernel extent outside 1..3, for extent + 2 padding
 *   + 2 dilation beyond 32-bit coordinates and for an output grid the index form refuses; U3D_EINVAL for stride / dilation < 1, padding
 *   < 0, an empty output level, NULL pointers, n <= 0 and a cap below min(n_in, n_out).  Added entry points: U3D_ABI_VERSION is unchanged.
 * ===================================================================================== */
int u3d_conv_out_shape(const int32_t* geom, int X, int Y, int Z, int32_t* out_shape);
int u3d_conv_mark(const int32_t* coords, int64_t n, const int32_t* geom, int B, int X, int Y, int Z, uint64_t* bitmap_out,
                  int64_t* cells_out, u3d_stream_t stream);
int u3d_conv_rulebook(const int32_t* out_coords, int64_t n_out, int64_t n_in, const uint64_t* bitmap_in, const int32_t* word_rank_in,
                      int64_t hash_slots, int B, int X, int Y, int Z, const int32_t* geom, int64_t cap, int32_t* pair_in,
                      int32_t* pair_out, int32_t* counts, void* ws, u3d_stream_t stream);
int64_t u3d_conv_rulebook_ws_bytes(int64_t n_out, int K);

/* =====================================================================================
 * R3t  Transposed convolution geometry (spconv's SparseConvTranspose3d): R3g's geom [12] plus outpad = int32 [3] on the HOST, the output
 *      padding.  Per axis out_dim = (in_dim - 1) s - 2 p + d (k - 1) + q + 1 (torch's rule); output cell o is active iff an active input
 *      i and a tap t in [0, k) give o = i s - p + t d on all three axes with 0 <= o < out_dim.  Offsets and weight layout as in R3g, taps
 *      not flipped.  (X, Y, Z) are the layer's INPUT extents.
 *   u3d_convt_out_shape (host only): out_shape int32 [3].
 *   u3d_convt_mark: the output occupancy of the n input rows, in u3d_conv_mark's two forms (bitmap_out sized by u3d_index_words(B,
 *     out_shape), or cells_out int64 [K n]); exactly one is non-NULL.
 *   The pair lists need no entry point of their own: o = i s - p + t d is R3g's relation with the two levels swapped, so
 *     u3d_conv_rulebook(out_coords = the layer's INPUT rows, the NEW level's index and extents, the same geom) returns them --
 *     pair_out = layer-input rows, pair_in = new-level rows, both ascending, at most min(n_in, n_out) pairs per offset.
 *   Errors, before any HIP call and with a u3d_last_error text: everything R3g's validation of k / s / p / d refuses; U3D_EINVAL for
 *   q < 0 or q >= max(s, d), for an empty output grid (an extent <= 0), NULL pointers and n <= 0; U3D_EUNSUPPORTED for an output extent
 *   (+ 2 padding + 2 dilation) beyond 32-bit coordinates, for an output grid the chosen index form cannot hold and for n K >= 2^31.
 *   Added entry points: U3D_ABI_VERSION is unchanged.
 * ===================================================================================== */
int u3d_convt_out_shape(const int32_t* geom, const int32_t* outpad, int X, int Y, int Z, int32_t* out_shape);
int u3d_convt_mark(const int32_t* coords, int64_t n, const int32_t* geom, const int32_t* outpad, int B, int X, int Y, int Z,
                   uint64_t* bitmap_out, int64_t* cells_out, u3d_stream_t stream);

/* tile_starts int32 [K, n_tiles+1]: lower bound of t*tile_rows in the (ascending) list rows[k][0..counts[k]). */
int u3d_tile_starts(const int32_t* rows, const int32_t* counts, int K, int64_t cap, int tile_rows,
                    int64_t n_tiles, int32_t* tile_starts, u3d_stream_t stream);

/* =====================================================================================
 * K4-K8  sparse convolution, all variants through one gather-MFMA-scatter kernel:
 *   dst[scatter[k][p]] (+)= W_k . src[gather[k][p]]      for p < counts[k], k < K
 * w_packed: the weights in the kernel's MFMA-fragment order, produced by u3d_weight_pack() from spconv's native
 * [C_out,k0,k1,k2,C_in] tensor (transposed = 0 for forward, 1 for the input gradient, where dst = C_in).
 * scatter lists must be ascending (they are, in both columns); tile_starts from u3d_tile_starts
 * on the scatter lists with the tile height u3d_spconv_plan() returns.  addend (nullable, [n_dst,Cd]) initialises the accumulator
 * (fuses the residual add of ResidualBlock.forward, spconv_unet.py:88-89).
 * Replaces SubMConv3d / SparseConv3d / SparseInverseConv3d forward and their input-gradients.
 * ===================================================================================== */
int u3d_spconv_gmm(const float* src, int64_t n_src, const float* w_packed, const int32_t* gather, const int32_t* scatter,
                   const int32_t* tile_starts, int K, int64_t cap, int Cs, int Cd, int64_t n_dst,
                   int tile_rows, int k_groups, const float* addend, float* dst, void* ws,
                   float* bn_partial /* nullable, k_groups == 1 only: float [ceil(n_dst / tile_rows)][2][Cd], per-tile sum x | sum x^2 of
                                        dst for the batch norm behind this convolution (u3d_bn_forward / u3d_bn_stats take it) */,
                   double flops_hint, u3d_stream_t stream);
/* bf16-operand form (BASELINE configs[2], "MFMA bf16 on rule GEMM"): same arguments; src / dst / addend stay fp32, gathered
 * rows are rounded to bf16 as the MFMA operand is formed, weights come pre-rounded from u3d_weight_pack_bf16 (Cd*K*Cs*2 bytes,
 * fragment order of v_mfma_f32_16x16x32_bf16); fp32 accumulation.  Cs % 32 == 0. */
int u3d_spconv_gmm_bf16(const float* src, int64_t n_src, const void* w_rows_bf16, const int32_t* gather, const int32_t* scatter,
                        const int32_t* tile_starts, int K, int64_t cap, int Cs, int Cd, int64_t n_dst, int tile_rows,
                        int k_groups, const float* addend, float* dst, void* ws, float* bn_partial, double flops_hint, u3d_stream_t stream);
int u3d_weight_pack_bf16(const float* w, void* wp, int Cd, int K, int Cs, int transposed, u3d_stream_t stream);
/* bf16 SOURCE ROWS (BASELINE configs[2] with bf16 copies of the gathered activations in HBM): src_bf16 is the shadow a
 * batch-norm call wrote next to its fp32 output (u3d_bn_apply / u3d_bn_bwd_apply, y_bf16 / dx_bf16): [n_src][Cs] bf16, rounded to
 * nearest even, each 32-channel group in MFMA fragment order (16 bytes at byte 16 q = channels 4q..4q+3, 16+4q..16+4q+3).  A lane
 * loads its fragment straight from the row: half the gathered bytes, no LDS transposition, no rounding arithmetic.  Weights from
 * u3d_weight_pack_bf16 (the same pack as u3d_spconv_gmm_bf16); dst / addend fp32, fp32 accumulation; results are bit-identical to
 * u3d_spconv_gmm_bf16 on the fp32 tensor the shadow was rounded from.  Always the workgroup-tile kernel (csrc/spconv_wg.hip). */
int u3d_spconv_gmm_bf16a(const void* src_bf16, int64_t n_src, const void* w_rows_bf16, const int32_t* gather, const int32_t* scatter,
                         const int32_t* tile_starts, int K, int64_t cap, int Cs, int Cd, int64_t n_dst, int tile_rows,
                         int k_groups, const float* addend, float* dst, void* ws, double flops_hint, u3d_stream_t stream);
/* fp32 products on the bf16 matrix pipe (see u3d_fp32_math): same arguments and results at fp32-level error; the gathered rows are
 * split exactly into three bf16 planes as the MFMA operand is formed, the weights come pre-split from u3d_weight_pack_x3
 * (Cd*K*Cs*6 bytes: three consecutive 1 KB plane blocks per (32-channel group, 16-column block) of the bf16 form's order), a
 * fragment pair takes six v_mfma_f32_16x16x32_bf16.  Cs % 32 == 0.  The host picks this form over u3d_spconv_gmm when
 * u3d_fp32_math(-1) == 1 -- the packed-weight layout belongs to the entry point, so the library does not switch it silently. */
int u3d_spconv_gmm_x3(const float* src, int64_t n_src, const void* w_rows_x3, const int32_t* gather, const int32_t* scatter,
                      const int32_t* tile_starts, int K, int64_t cap, int Cs, int Cd, int64_t n_dst, int tile_rows,
                      int k_groups, const float* addend, float* dst, void* ws, float* bn_partial, double flops_hint, u3d_stream_t stream);
int u3d_weight_pack_x3(const float* w, void* wp, int Cd, int K, int Cs, int transposed, u3d_stream_t stream);
/* ---- forward convolution with an OUTPUT EPILOGUE (fused inference: eval-mode batch norm + ReLU, the U-Net's concat buffer).
 * The four launches above in one entry point -- fmt 0: u3d_spconv_gmm, 1: _bf16, 2: _x3, 3: _bf16a (src = bf16 rows); same kernels,
 * same packed weights, same sums -- whose dst rows leave the accumulator tile through the host struct below instead of into dst.
 * With x the fp32 value the plain launch stores (after the addend, after the fixed-order sum over offset groups):
 *   raw (nullable)          raw[row * raw_ld + raw_col + c] = x[row][c]: dst as a column block of a wider buffer;
 *   act[j], j < n_act <= 2  act[j][row * act_ld[j] + act_col[j] + c] = f(x[row][c] * scale[j][act_col[j] + c] + shift[j][act_col[j] + c]),
 *                           f = max(., 0) where relu[j], else the identity: u3d_bn_apply's expression and rounding, bit for bit.
 *                           scale / shift are indexed by the column of act[j] itself, so a norm over a wider tensor is applied to its
 *                           column blocks by the launches that produce them.
 * Contract: at least one output; every ld >= col + Cd, every ld and col a multiple of 4 floats (16-byte vector stores only), otherwise
 * U3D_EINVAL; n_act outside [0, 2], or bn_partial non-NULL (the statistics epilogue of training and this one exclude each other):
 * U3D_EUNSUPPORTED -- each with a u3d_last_error text and before any launch.  tile_rows in {32, 64} and k_groups in {1} (any K) or
 * {3, 9} (K >= 27) are the CALLER'S choice here (u3d_spconv_plan[_bf16a] give the measured ones); ws = k_groups * n_dst * Cd * 4 bytes
 * when k_groups > 1 -- the main kernel then writes partials as always and the epilogue runs in the reduce.  addend is [n_dst][Cd].
 * Outputs must not overlap each other or the inputs.  Added entry point: U3D_ABI_VERSION is unchanged.
 * relu[j] is a FLAG WORD: U3D_EP_RELU = the ReLU follows; U3D_EP_BF16_ROWS = act[j] is a bf16-ROW buffer, the shadow u3d_bn_apply writes
 * (y_bf16) and u3d_spconv_gmm_bf16a / fmt 3 gather: the same value rounded to nearest even, each 32-channel group in fragment order (the
 * 8-byte piece of channels 4q..4q+3 of 16-channel half h at piece 2q + h), one 8-byte store per four channels.  For such an output act_ld[j]
 * and act_col[j] count bf16 ELEMENTS and, like Cd, must be multiples of 32 (else U3D_EINVAL); scale / shift stay fp32, indexed by the
 * output's own column.  No fp32 copy is written: a norm that is wanted in both forms takes two slots with the same scale / shift.  Any other
 * bit: U3D_EUNSUPPORTED.  u3d_spconv_gmm_ep_formats() (host only) tells what the library writes -- bit 0: fp32 activated outputs, bit 1:
 * bf16-row ones; a caller must see bit 1 before it sets U3D_EP_BF16_ROWS (a library from before the flag reads any non-zero word as "ReLU"
 * and would write fp32 into the bf16 buffer; it lacks this symbol). */
#define U3D_EP_RELU 1
#define U3D_EP_BF16_ROWS 2
typedef struct u3d_conv_epilogue {
    float* raw;
    int64_t raw_ld, raw_col;
    int n_act;
    float* act[2];
    const float* scale[2];
    const float* shift[2];
    int64_t act_ld[2], act_col[2];
    int relu[2];
} u3d_conv_epilogue;
int u3d_spconv_gmm_ep(int fmt, const void* src, int64_t n_src, const void* w_rows, const int32_t* gather, const int32_t* scatter,
                      const int32_t* tile_starts, int K, int64_t cap, int Cs, int Cd, int64_t n_dst, int tile_rows,
                      int k_groups, const float* addend, void* ws, float* bn_partial, const u3d_conv_epilogue* ep, double flops_hint,
                      u3d_stream_t stream);
int u3d_spconv_gmm_ep_formats(void);
/* all packs of a model in one launch: desc = device array of n_desc records of eight int64
 * {src pointer, dst pointer, Cd, K, Cs, transposed, format (0 fp32, 1 bf16, 2 x3), first block}; record i owns blocks
 * [first_i, first_{i+1}) of 256 threads: one 16-byte output vector per thread in the fp32 (Cd*K*Cs/4 threads) and bf16 (Cd*K*Cs/8)
 * forms, the three plane vectors of one bf16-form position per thread in the x3 form (Cd*K*Cs/8 threads). */
int u3d_weight_pack_batch(const void* desc, int n_desc, int64_t total_blocks, u3d_stream_t stream);
/* Launch plan for a shape: tile_rows (rows per wave-tile = the tile height to pass to u3d_tile_starts) and
 * k_groups (kernel offsets are split into that many groups when the level has too few rows to fill the chip;
 * the groups' partial sums go through ws = k_groups*n_dst*Cd*4 bytes and a fixed-order reduce).
 * Channel contract of the sparse convolutions (forward, input gradient, weight gradient): Cs in {16} u {32, 64, ..., 512},
 * Cd in {32, 64, ..., 512}; U3D_EUNSUPPORTED for anything else, before any HIP call.  The widths of the 32-channel five-level U-Net
 * (Cs / 16 in {1, 2, 4, 6, 8, 10, 12, 16}) run fully unrolled kernels, every other width a run-time loop over 32 / 64 / 128-channel
 * chunks of the source row; the weight gradient has 17 whole-block (Cs, Cd) kernels and a channel-blocked walk for the rest. */
int u3d_spconv_plan(int Cs, int Cd, int K, int64_t n_dst, int* tile_rows, int* k_groups);
/* the plan u3d_spconv_gmm_bf16a wants (its light items prefer 32-row tiles and fewer offset groups at the small levels) */
int u3d_spconv_plan_bf16a(int Cs, int Cd, int K, int64_t n_dst, int* tile_rows, int* k_groups);
/* 1 where u3d_spconv_gmm_bf16a has a kernel for the source width (those of the 32-channel five-level U-Net: Cs in {32, 64, 96, 128, 160,
 * 192, 256}), else 0: the caller then gathers the fp32 rows with bf16 operands (u3d_spconv_gmm_bf16) -- same operands, same results. */
int u3d_spconv_gmm_bf16a_supported(int Cs, int Cd);
/* ---- tile-stationary SubMConv3d(k=3) (csrc/spconv_ts.hip; unidet3d/spconv_unet.py:43-56): accumulators of a row tile in registers
 * for all 27 offsets and all C_out columns, every source row of a tile fetched once.
 * u3d_subm_halo builds, per tile of tile_rows consecutive rows (64 / 128 / 256) of a level, from the same occupancy index the
 * rulebook uses:  nhalo int32 [n_tiles]; halo int32 [n_tiles][27*tile_rows] -- the sorted unique source rows of the tile's
 * (row, offset) neighbours, the first nhalo[t] entries valid;  loc uint16 [n_tiles][27][tile_rows] -- position of neighbour k of
 * row r in that list, 0xFFFF = none;  pmask uint32 [n_tiles][pmax] -- bit k of word p: offset k has a neighbour among entries
 * [p*halo_rows, (p+1)*halo_rows) of the list (pmax = u3d_subm_halo_pmax(tile_rows, halo_rows) <= 64).  Integer-only, deterministic.
 * u3d_spconv_ts_x3: dst[r] = addend[r] + sum_k W_k' . src[neighbour_k(r)] with fp32 products from three bf16 planes (weights from
 * u3d_weight_pack_x3, K = 27); flip = 0: k' = k (forward); flip = 1: k' = 26 - k with the TRANSPOSED pack -- the input gradient
 * (SubM pairs are symmetric).  tile_rows / halo_rows must be the pair the tables were built for (u3d_spconv_ts_plan gives the
 * measured choice per shape, U3D_EUNSUPPORTED for shapes the kernel is not instantiated for -- the caller then uses u3d_spconv_gmm_x3). */
/* Register-stationary form of the same convolution (csrc/spconv_ts.hip spconv_rs_k): persistent workgroups (`workgroups` of them, <= 0:
 * one per CU) keep the weights of all 27 offsets of a 32 -> 32 channel block in registers for the whole launch -- each of the four
 * waves the fragments of its 6-7 offsets -- and walk contiguous ranges of 64-row tiles: no weight traffic and no barrier per offset;
 * the waves' partial tiles are added in wave order (deterministic).  Wider layers run as Cs/32 x Cd/32 launches of the block kernel
 * inside this call (accumulating over the source blocks).  Tables: u3d_subm_halo(..., tile_rows = 64, halo_rows) with halo_rows in
 * {256, 320, 416} (tiles with more unique source rows take further passes); pmask is not read.  Same arguments otherwise. */
int u3d_spconv_rs_x3(const float* src, int64_t n, const void* w_rows_x3, const int32_t* nhalo, const int32_t* halo, const uint16_t* loc,
                     int halo_rows, int flip, int Cs, int Cd, const float* addend, float* dst, int workgroups, double flops_hint, u3d_stream_t stream);
/* bf16-operand form of u3d_spconv_rs_x3 on bf16 ROWS (the shadows of u3d_spconv_gmm_bf16a; weights from u3d_weight_pack_bf16): one plane,
 * no split, 56 weight registers per wave -- three workgroups per CU (`workgroups` <= 0: 3 per CU).  halo_rows in {256, 320, 448}. */
int u3d_spconv_rs_bf16a(const void* src_bf16, int64_t n, const void* w_rows_bf16, const int32_t* nhalo, const int32_t* halo, const uint16_t* loc,
                        int halo_rows, int flip, int Cs, int Cd, const float* addend, float* dst, int workgroups, double flops_hint, u3d_stream_t stream);
int u3d_spconv_ts_plan(int Cs, int Cd, int64_t n, int* tile_rows, int* halo_rows);
int u3d_subm_halo_pmax(int tile_rows, int halo_rows);
int u3d_subm_halo(const int32_t* coords, int64_t n, const uint64_t* bitmap, const int32_t* word_rank, int64_t hash_slots, int B,
                  int X, int Y, int Z, int tile_rows, int halo_rows, int32_t* nhalo, int32_t* halo, uint16_t* loc, uint32_t* pmask,
                  u3d_stream_t stream);
int u3d_spconv_ts_x3(const float* src, int64_t n, const void* w_rows_x3, const int32_t* nhalo, const int32_t* halo, const uint16_t* loc,
                     const uint32_t* pmask, int tile_rows, int halo_rows, int flip, int Cs, int Cd, const float* addend, float* dst,
                     double flops_hint, u3d_stream_t stream);
/* dW[(n*K+k)*Cs + c] = sum_p dy[rows_dy[k][p]][n] * x[rows_x[k][p]][c]   (dW is overwritten).
 * The pairs of offset k are processed per tile of dy rows: tile_starts = u3d_tile_starts(rows_dy, ..., tile_rows =
 * u3d_spconv_wgrad_tile_rows(...)); per-tile partial blocks go through ws and are summed in a fixed order
 * (deterministic, no atomics).
 * Both conv entry points address through 32-bit buffer offsets: row counts < 2^24, feature matrices and pair lists < 2 GiB
 * (U3D_EUNSUPPORTED otherwise). */
int u3d_spconv_wgrad(const float* x, int64_t n_rows_x, const float* dy, const int32_t* rows_x, const int32_t* rows_dy,
                     const int32_t* tile_starts, int K, int64_t cap, int64_t n_rows_dy, int tile_rows, int Cs, int Cd,
                     float* dW, void* ws, double flops_hint, u3d_stream_t stream);
/* bf16-operand form (BASELINE configs[2]): x and dy rows are rounded to bf16 as the v_mfma_f32_16x16x32_bf16 operands are
 * formed (32 pairs per instruction); fp32 accumulation, partials and reduce.  Same arguments / workspace. */
int u3d_spconv_wgrad_bf16(const float* x, int64_t n_rows_x, const float* dy, const int32_t* rows_x, const int32_t* rows_dy,
                          const int32_t* tile_starts, int K, int64_t cap, int64_t n_rows_dy, int tile_rows, int Cs, int Cd,
                          float* dW, void* ws, double flops_hint, u3d_stream_t stream);
/* Weight gradient from bf16 ROWS: x_bf16 / dy_bf16 are the shadows u3d_bn_apply (y_bf16) and u3d_bn_bwd_apply (dx_bf16) wrote --
 * [n][C] bf16 in fragment order (see u3d_spconv_gmm_bf16a).  Whole rows are gathered, turned in LDS with ds_read_b64_tr_b16 and
 * multiplied by v_mfma_f32_16x16x32_bf16 (32 pairs per instruction), fp32 accumulation, fixed-order reductions; dW comes out in
 * the natural [C_out][K][C_in] layout.  Same tile plan and workspace as u3d_spconv_wgrad.  Instantiated for 32 / 64 channels (one wave per tile)
 * and the twelve 64 ... 256-channel combinations of levels 3-5 and the tail blocks (four waves share a tile): ask
 * u3d_spconv_wgrad_rows_supported; the operands are the bf16 values, so the result equals u3d_spconv_wgrad on the rounded tensors
 * up to fp32 summation order. */
int u3d_spconv_wgrad_rows(const void* x_bf16, int64_t n_rows_x, const void* dy_bf16, const int32_t* rows_x, const int32_t* rows_dy,
                          const int32_t* tile_starts, int K, int64_t cap, int64_t n_rows_dy, int tile_rows, int Cs, int Cd,
                          float* dW, void* ws, double flops_hint, u3d_stream_t stream);
int u3d_spconv_wgrad_rows_supported(int Cs, int Cd);
int u3d_spconv_wgrad_tile_rows(int K, int64_t n_rows_dy, int Cs, int Cd);
int64_t u3d_spconv_wgrad_ws_bytes(int K, int64_t n_rows_dy, int Cs, int Cd);
/* wp = fragment-ordered copy of the weights for u3d_spconv_gmm ([Cd*K*Cs] floats):
 * transposed = 0: logical W(n,k,c) = w[(n*K+k)*Cs + c]; transposed = 1: W(n,k,c) = w[(c*K+k)*Cd + n]. */
int u3d_weight_pack(const float* w, float* wp, int Cd, int K, int Cs, int transposed, u3d_stream_t stream);
/* wt[(c*K + k)*Cd + n] = w[(n*K + k)*Cs + c] */
int u3d_weight_transpose(const float* w, float* wt, int Cd, int K, int Cs, u3d_stream_t stream);

/* =====================================================================================
 * K9  BatchNorm1d / SyncBatchNorm (train) + ReLU over voxel rows
 *     (unidet3d/spconv_unet.py:42,49,119-124,147,177; unidet3d/unidet3d.py:104-111).
 *     Split so that the caller can all-reduce the fp64 statistics between the two phases
 *     (SyncBatchNorm across data-parallel ranks).
 * ===================================================================================== */
/* sums[0..C) = sum x, sums[C..2C) = sum x^2, sums[2C] = n (fp64): per-workgroup partial rows in ws, added in a fixed order by a
 * second launch -> deterministic.  partial != NULL: the statistics come from the per-tile sums a convolution epilogue wrote
 * (u3d_spconv_gmm bn_partial, float [n_tiles][2][C]) and x is not read.  ws: u3d_bn_ws_bytes(C). */
int u3d_bn_stats(const float* x, int64_t n, int C, const float* partial, int64_t n_tiles, double* sums, void* ws, u3d_stream_t stream);
int64_t u3d_bn_ws_bytes(int C);
/* mean/var from sums/count; scale = gamma*invstd, shift = beta - mean*scale; running stats updated in place
 * (momentum, unbiased var) when running_mean != NULL.  count <= 0: the row count is read from sums[2C]
 * (it then travels through the SyncBatchNorm all-reduce with the sums: no host read-back).
 * num_batches_tracked (nullable, device int64 scalar) is incremented by one. */
int u3d_bn_finalize(const double* sums, double count, const float* gamma, const float* beta, float eps,
                    float momentum, float* running_mean, float* running_var, int C, float* mean, float* invstd,
                    float* scale, float* shift, int64_t* num_batches_tracked, u3d_stream_t stream);
/* y_bf16 (nullable, [n][C] bf16, C % 32 == 0): a copy of y rounded to nearest even, fragment order inside each 32-channel group
 * (see u3d_spconv_gmm_bf16a), written in the same pass -- the source rows of u3d_spconv_gmm_bf16a. */
int u3d_bn_apply(const float* x, const float* scale, const float* shift, int relu, int64_t n, int C, float* y, void* y_bf16,
                 u3d_stream_t stream);
/* backward of y = relu(x*scale+shift): sums[0..C) = sum dy', sums[C..2C) = sum dy'*xhat  (dy' = dy*[y>0]);
 * sums[2C] is left untouched (the caller keeps the forward row count there). */
int u3d_bn_bwd_stats(const float* x, const float* dy, const float* mean, const float* invstd,
                     const float* scale, const float* shift, int relu, int64_t n, int C, double* sums, void* ws, u3d_stream_t stream);
/* dx = scale*(dy' - sum_dy/count - xhat*sum_dyxhat/count); dgamma = sum_dyxhat, dbeta = sum_dy (fp32 out);
 * count <= 0: read from sums[2C]. */
int u3d_bn_bwd_apply(const float* x, const float* dy, const float* mean, const float* invstd,
                     const float* scale, const float* shift, int relu, const double* sums, double count,
                     int64_t n, int C, float* dx, void* dx_bf16 /* nullable [n][C] bf16: dx rounded to nearest even (as y_bf16 of u3d_bn_apply) */,
                     float* dgamma, float* dbeta, const float* addend /* nullable [n][C]: added to dx (a second gradient of x, e.g. the residual identity branch) */,
                     u3d_stream_t stream);

/* Single-call forms for the non-distributed case: forward = statistics -> sum + finalize -> apply; backward = bwd_stats -> sum ->
 * bwd_apply.  st float [4C] = mean, invstd, scale, shift (saved for backward); sums double [2C+1]; partial / n_tiles as in
 * u3d_bn_stats. */
int u3d_bn_forward(const float* x, int64_t n, int C, const float* partial, int64_t n_tiles, const float* gamma, const float* beta, float eps,
                   float momentum, float* running_mean, float* running_var, int64_t* num_batches_tracked, int relu, float* y, void* y_bf16 /* nullable */,
                   float* st, double* sums, void* ws, u3d_stream_t stream);
/* fwd_sums: the forward call's sums vector (its entry [2C] is the row count the backward divides by) */
int u3d_bn_backward(const float* x, const float* dy, const float* st, int relu, const double* fwd_sums, double* sums, int64_t n,
                    int C, float* dx, void* dx_bf16 /* nullable */, float* dgamma, float* dbeta, const float* addend /* nullable, as in u3d_bn_bwd_apply */,
                    void* ws, u3d_stream_t stream);

/* =====================================================================================
 * K11/K12  superpoint pooling -- replaces x.features[inverse_mapping] + torch_scatter.scatter_mean
 *     (unidet3d/unidet3d.py:130) and the superpoint centres (:332-333, :446-447).
 * ===================================================================================== */
/* CSR of element ids per segment: offsets int32 [S+1], list int32 [L], element ids ASCENDING inside every segment (stable radix
 * sort of the ids by segment id, csrc/radix.hip): the sums the pooling kernels take over a segment then have one order, so pooled
 * features -- and with them the whole training step -- are bit-reproducible from run to run. */
int u3d_csr_build(const int64_t* seg_ids, int64_t L, int64_t S, int32_t* offsets, int32_t* list, void* ws,
                  u3d_stream_t stream);
int64_t u3d_csr_build_ws_bytes(int64_t L, int64_t S);
/* out[j] = map[list[j]]  (int64 map -> int32) : composes the CSR with inverse_mapping / superpoint ids */
int u3d_gather_i64_to_i32(const int64_t* map, const int32_t* list, int64_t L, int32_t* out, u3d_stream_t stream);
/* out[s] = out_scale(s) * sum_{j in [offsets[s],offsets[s+1])} src_scale(rows[j]) * src[rows[j]]
 * mean_mode 1: out_scale = 1/max(len,1) (scatter_mean semantics: empty segment -> 0).
 * src_inv_count (nullable, int32 [n_src rows' segment sizes]) : src_scale(r) = 1/max(src_inv_count[r+1]-src_inv_count[r],1)
 * (backward of the mean: rows are superpoints, scaled by their own 1/count). */
int u3d_segment_gather_sum(const float* src, const int32_t* rows, const int32_t* offsets, int64_t S, int C,
                           int mean_mode, const int32_t* src_seg_offsets, float* out, u3d_stream_t stream);
/* centres[s] = mean over the segment's points of (xyz - sub[scene]) ; points row stride pt_ld floats.
 * sub (nullable) [B, sub_ld] holds the per-scene shift (the voxelizer's stats rows: min xyz), the scene
 * of a segment is found from its first point via pt_offsets int64 [B+1]. */
int u3d_segment_mean_xyz(const float* points, int pt_ld, const int32_t* list, const int32_t* offsets, int64_t S,
                         const float* sub, int sub_ld, const int64_t* pt_offsets, int B, float* out,
                         u3d_stream_t stream);

/* out[s] = [min xyz, max xyz] of (xyz - sub[scene]) over the points with ids[p] == s (ids < 0 are skipped):
 * the axis-aligned GT boxes of UniDet3D.get_bboxes_by_masks (unidet3d/unidet3d.py:220-256) for a whole batch in one
 * pass.  A segment without points returns NaN in all six components, whichever chunk of segments holds it (the untouched
 * ordered keys INT_MAX / INT_MIN decode to the bit patterns 0x7fffffff / 0xffffffff): an absent instance is loud, not a box of
 * plausible size.  ws: n_seg*6*4 bytes. */
int u3d_segment_minmax_xyz(const float* points, int pt_ld, const int64_t* ids, int64_t n, int n_seg, const float* sub,
                           int sub_ld, const int64_t* pt_offsets, int B, float* out /*[n_seg,6]*/, void* ws,
                           u3d_stream_t stream);

/* =====================================================================================
 * P1  Sparse max / average pooling over a convolution rulebook (spconv's SparseMaxPool3d / SparseAvgPool3d; csrc/sparse_pool.hip).
 *     Geometry: R3g's, offsets in the order (t0 k1 + t1) k2 + t2; every output row has at least one pair.
 *   u3d_pair_table: the destination-major view of K pair lists.  pair_key / pair_val int32 [K, cap], counts int32 [K]; table int32
 *     [n, K] receives table[pair_key[k][i]][k] = pair_val[k][i] for i < counts[k] and -1 everywhere else (every entry is written;
 *     4 K n bytes).  Race-free because for a fixed offset no row repeats (u3d_conv_rulebook).  With (key, val) = (pair_out, pair_in),
 *     n = n_out it gives each output row its inputs, with (pair_in, pair_out), n = n_in each input row its outputs.
 *   u3d_sparse_pool_fwd (x [n_in, C], table_out [n_out, K]):
 *     max: y[j, c] = the maximum over the inputs PRESENT in the window of j -- an absent cell is not a zero.  Selection: walk the offsets
 *       in ascending index; take the first value; replace the held value only if the new one is > it, or if the new one is NaN and the
 *       held one is not.  So the first maximal element wins a tie, +0.0 and -0.0 do not replace each other, a NaN in the window gives NaN.
 *       y holds the BITS of the selected element, arg uint8 [n_out, C] its offset index.  count is not touched.
 *     avg: y[j, c] = (sum of the present inputs in ascending offset order) / count[j]; count int32 [n_out] receives the number of pairs of
 *       each row.  arg is not touched.
 *   u3d_sparse_pool_bwd (dy [n_out, C], table_in [n_in, K]), every dx element written once (an input row without outputs gets 0):
 *     max: dx[i, c] = sum over the offsets k, ascending, of dy[j_k, c] for the outputs j_k = table_in[i][k] with arg[j_k, c] == k: a tie
 *       sends the gradient to the one selected element (torch's dense rule).
 *     avg: dx[i, c] = sum over k, ascending, of dy[j_k, c] * (1 / count[j_k]).
 *   No floating-point atomics, one summation order: results are bit-reproducible.  The unused one of arg / count may be NULL.
 *   Contract: C % 4 == 0, 4 <= C <= 512, 1 <= K <= 27, mode U3D_POOL_MAX or U3D_POOL_AVG; rows past n are not touched.  Errors, before
 *   any HIP call and with a u3d_last_error text: U3D_EINVAL for NULL pointers, n <= 0, cap <= 0 and an unknown mode; U3D_EUNSUPPORTED
 *   for other widths or offset counts and for n max(C, K) >= 2^31.  Added entry points: U3D_ABI_VERSION is unchanged.
 * ===================================================================================== */
#define U3D_POOL_MAX 0
#define U3D_POOL_AVG 1
int u3d_pair_table(const int32_t* pair_key, const int32_t* pair_val, const int32_t* counts, int K, int64_t cap, int64_t n, int32_t* table,
                   u3d_stream_t stream);
int u3d_sparse_pool_fwd(const float* x, const int32_t* table_out, int64_t n_out, int K, int C, int mode, float* y,
                        uint8_t* arg /* max only */, int32_t* count /* avg only */, u3d_stream_t stream);
int u3d_sparse_pool_bwd(const float* dy, const int32_t* table_in, int64_t n_in, int K, int C, int mode, const uint8_t* arg /* max only */,
                        const int32_t* count /* avg only */, float* dx, u3d_stream_t stream);

/* =====================================================================================
 * B1  Bias of the sparse convolution layers (bias=True; csrc/sparse_bias.hip).  y, dy fp32 [n, C]; bias, db fp32 [C].
 *   u3d_bias_add: y[r, c] += bias[c] in place over every row: one fp32 addition per element, the bits of y + b.
 *   u3d_bias_grad: db[c] = sum over the rows of dy[r, c].  Two passes: workgroup b sums the fixed row range [b R, (b + 1) R),
 *     R = U3D_BIAS_GRAD_ROWS, in fp64 into ws; then the partials of a channel are added in fp64 -- lane l of a wave takes l, l + S, ...
 *     (S = U3D_BIAS_GRAD_STEP) in ascending order, a fixed tree adds the lanes -- and the sum is rounded once to fp32.  No atomics, one
 *     summation order: bit-identical from run to run.  ws: u3d_bias_grad_ws_bytes(n, C) = ceil(n / R) C doubles.
 *   Contract: C % 32 == 0, 32 <= C <= 512 (the convolution's destination widths), 1 <= n < 2^31; rows past n are not touched.  Errors,
 *   before any HIP call and with a u3d_last_error text: U3D_EINVAL for NULL pointers and n <= 0, U3D_EUNSUPPORTED for other widths and
 *   row counts.  n == 0 is the caller's business (no launch; db = 0).  Added entry points: U3D_ABI_VERSION is unchanged.
 * ===================================================================================== */
#define U3D_BIAS_GRAD_ROWS 512
#define U3D_BIAS_GRAD_STEP 64
int u3d_bias_add(float* y, const float* bias, int64_t n, int C, u3d_stream_t stream);
int u3d_bias_grad(const float* dy, int64_t n, int C, float* db, void* ws, u3d_stream_t stream);
int64_t u3d_bias_grad_ws_bytes(int64_t n, int C);

/* =====================================================================================
 * A1  Stand-alone ReLU of a sparse layer stack: an nn.ReLU that no batch norm precedes (csrc/relu.hip).  Flat fp32 buffers of `count`
 *     elements, any count >= 1: every row count and channel count a layer can produce.  Not on the hot path.
 *   u3d_relu_fwd: y[i] = x[i] > 0 ? x[i] : +0.0 (so -0.0 and NaN give +0.0).
 *   u3d_relu_bwd: dx[i] = x[i] > 0 ? dy[i] : +0.0: the bits of dy where the unit is on, no arithmetic.
 *   Every element written once; y / dx may be x / dy themselves.  Errors, before any HIP call and with a u3d_last_error text: U3D_EINVAL
 *   for NULL pointers and count <= 0 (an empty tensor is the caller's business: no launch).  Added entry points: U3D_ABI_VERSION is unchanged.
 * ===================================================================================== */
int u3d_relu_fwd(const float* x, int64_t count, float* y, u3d_stream_t stream);
int u3d_relu_bwd(const float* x, const float* dy, int64_t count, float* dx, u3d_stream_t stream);

/* =====================================================================================
 * S1  Sparse tensors on different voxel sets: union add and pruning (csrc/sparse_sets.hip).  Rows fp32 [n, C]; row maps int32.
 *   u3d_index_rows: rows_out[i] = the canonical row of coords[i] = (b, x, y, z) in the occupancy index (either form, as every entry
 *     point takes it), or -1 for a cell that is absent, outside the grid or outside the batch [0, B).  Thread = row.
 *   u3d_mask_compact: mask uint8 [n] (a torch.bool tensor's bytes; non-zero = keep).  kept int32 [n] receives the kept rows in ascending
 *     order in its first n_kept entries (the rest is not touched), pos int32 [n] the position of every row in that list or -1 (every
 *     entry written), n_kept int32 [1] the count.  Block counts, a scan of the block counts, a wave-64 ballot prefix inside each block:
 *     stable, no atomics, one result.  ws: u3d_mask_compact_ws_bytes(n) = (2 ceil(n / 256) + 64) * 4 bytes; 0 for n <= 0.
 *   u3d_rows_take: y[j] = x[rows[j]] for j < n_out, bit for bit; a row value outside [0, n_src) (unsigned compare: -1, n_src, anything)
 *     gives a row of +0.0.  Serves a gather by the kept list, a scatter read through the position list, and int32 [n, 4] coordinate
 *     rows viewed as C = 4 (16-byte moves: the bits are not touched).
 *   u3d_rows_take2: y[j] = a[rows_a[j]] + b[rows_b[j]] in one pass: the fp32 sum (one rounding) where both rows are present, the BITS of
 *     the present row where one is (-0.0 stays -0.0, a NaN keeps its payload), +0.0 where neither is.  Absent: as above, against n_a / n_b.
 *   Every destination element is written exactly once: no atomics, no memset, results are bit-reproducible.  Rows past n_out are not
 *   touched.  y must not overlap an input.
 *   Contract: C % 4 == 0, 4 <= C <= 512, every count < 2^31.  Errors, before any HIP call and with a u3d_last_error text: U3D_EINVAL
 *   for NULL pointers, n <= 0 / n_out <= 0, a negative source count and (u3d_index_rows) an empty grid; U3D_EUNSUPPORTED for other widths
 *   and for counts >= 2^31.  Empty inputs are the caller's business (no launch).  Added entry points: U3D_ABI_VERSION is unchanged.
 * ===================================================================================== */
int u3d_index_rows(const int32_t* coords, int64_t n, const uint64_t* bitmap, const int32_t* word_rank, int64_t hash_slots, int B, int X, int Y,
                   int Z, int32_t* rows_out, u3d_stream_t stream);
int u3d_mask_compact(const uint8_t* mask, int64_t n, int32_t* kept, int32_t* pos, int32_t* n_kept, void* ws, u3d_stream_t stream);
int64_t u3d_mask_compact_ws_bytes(int64_t n);
int u3d_rows_take(const float* x, const int32_t* rows, int64_t n_out, int64_t n_src, int C, float* y, u3d_stream_t stream);
int u3d_rows_take2(const float* a, const int32_t* rows_a, int64_t n_a, const float* b, const int32_t* rows_b, int64_t n_b, int64_t n_out, int C,
                   float* y, u3d_stream_t stream);

/* =====================================================================================
 * S2  Dense interchange of sparse tensors (csrc/sparse_dense.hip): SparseConvTensor.dense / from_dense.  Rows fp32 [n, C]; coords int32
 *     [n, 4] = (b, x, y, z); the dense grid is fp32 [B, X, Y, Z, C] (channels_first == 0) or [B, C, X, Y, Z] (channels_first != 0),
 *     contiguous.  Dense cell number of (b, x, y, z) = ((b X + x) Y + y) Z + z, a 32-bit number: B X Y Z < 2^31.  Element offsets are
 *     64-bit.  Every kernel is a copy: -0.0 stays -0.0, a NaN keeps its payload; every destination element is written exactly once, no
 *     atomics, no memset; results are bit-reproducible.
 *   u3d_dense_scatter: dense[cell] = feats[row of the cell in the occupancy index] (either form, as every entry point takes it), +0.0
 *     for a cell without a row.  Cell-driven: the zeros cost no second pass.  A looked-up row outside [0, n) is an absent row.
 *     Channels last: a group of lanes per cell, 16-byte slices.  Channels first: a workgroup owns 64 consecutive cell numbers of ONE
 *     batch item x 64 channels, rows read as 16-byte slices into a padded LDS tile, written out as 256-byte runs per channel.
 *   u3d_dense_gather: rows[i] = dense[cell of coords[i]]; a coordinate outside the grid or the batch [0, B) (unsigned compare) gives a
 *     row of +0.0 and reads nothing.  Row-driven: no index, no empty region touched.  Channels first: 64 consecutive rows x 64 channels
 *     through the same tile.
 *   u3d_dense_active: mask uint8 [n_cells] (a torch.bool tensor's bytes): 1 where any of the C values of cell i of a channels-last
 *     grid x [n_cells, C] is != 0 (a NaN is; -0.0 is not), else 0.  Every byte written.
 *   u3d_cells_coords: coords[i] = (b, x, y, z) of the dense cell number cells[i], one 16-byte store per row (no B: b = cell / (X Y Z)).
 *   Contract: C % 4 == 0, 4 <= C <= 512; 1 <= n, n_cells < 2^31; B, X, Y, Z >= 1.  Errors, before any HIP call and with a
 *   u3d_last_error text: U3D_EINVAL for NULL pointers, n <= 0 / n_cells <= 0, an empty grid, negative hash_slots; U3D_EUNSUPPORTED for
 *   other widths, counts or grids of 2^31 and more, and a launch of 2^24 workgroups and more.  Empty inputs are the caller's business
 *   (no launch).  Outputs must not overlap the inputs.  Added entry points: U3D_ABI_VERSION is unchanged.
 * ===================================================================================== */
int u3d_dense_scatter(const float* feats, int64_t n, int C, const uint64_t* bitmap, const int32_t* word_rank, int64_t hash_slots, int B, int X,
                      int Y, int Z, int channels_first, float* dense, u3d_stream_t stream);
int u3d_dense_gather(const float* dense, int B, int X, int Y, int Z, int C, int channels_first, const int32_t* coords, int64_t n, float* rows,
                     u3d_stream_t stream);
int u3d_dense_active(const float* x, int64_t n_cells, int C, uint8_t* mask, u3d_stream_t stream);
int u3d_cells_coords(const int32_t* cells, int64_t n, int X, int Y, int Z, int32_t* coords, u3d_stream_t stream);

/* =====================================================================================
 * S3  Per-scene operations on sparse tensors (csrc/sparse_scene.hip): scene ranges, top-k per scene, global max / average pooling.
 *     coords int32 [n, 4] = (b, x, y, z) in canonical order, so the batch index ascends; rows fp32 [n, C]; offsets int32 [B + 1].
 *   u3d_scene_offsets: offsets[b] = the first row whose batch index is >= b, offsets[B] = n; empty scenes at the start, in the middle
 *     and at the end come out right.  Thread = row: it compares its batch index with its predecessor's and writes every entry in
 *     between, so each entry is written exactly once (no atomics on offsets, no memset of it).  flag int32 [1] (cleared by the call):
 *     bit 0 = a batch index descends, bit 1 = a batch index lies outside [0, B).  A flagged tensor is not in canonical order; its
 *     offsets are unspecified, and every reader below clamps the ranges it takes from them to [0, n]: wrong values, never an access
 *     outside a tensor.
 *   u3d_scene_topk: scene b keeps its first min(k[b], n_b) rows in this order: key descending, then row ascending.  key = the
 *     order-preserving integer image of the score's bits: every NaN is one key above +inf, -0.0 equals +0.0, denormals keep their value
 *     (no floating-point instruction reads a score).  largest == 0 reverses the order of the numbers only: NaNs still come first, ties
 *     still go to the lower row.  k int32 [B] on the device; a negative entry counts as 0.  Outputs: mask uint8 [n] (a torch.bool
 *     tensor's bytes, every byte written), kept int32 [n] (the kept rows ascending in the first n_kept entries, the rest not touched),
 *     pos int32 [n] (the position of every row in that list or -1, every entry written), result int32 [2] = (n_kept, the flag word of
 *     u3d_scene_offsets): one host read serves both.  A radix select: four 8-bit histogram passes over the keys of each scene
 *     (blocks_per_scene workgroups per scene, LDS counters, one integer atomic per non-empty bin and workgroup) give the threshold key T
 *     and the rows strictly above it; one stable pass keeps key > T plus the first k - above rows with key == T (block counts, a scan,
 *     a wave-64 ballot prefix).  Integer only, no floating-point atomic: one result whatever the arrival order.
 *     ws: u3d_scene_topk_ws_bytes(n, B) bytes (0 for n <= 0 or B <= 0); the call clears what it needs of it.
 *   u3d_scene_topk_plan (host only): rows_per_block = the rows one workgroup takes per trip of a histogram pass (and of a block of the
 *     stable pass), blocks_per_scene = the workgroups per scene: a scene of more than rows_per_block * blocks_per_scene rows takes a
 *     second trip.  Either pointer may be NULL.
 *   u3d_scene_pool_fwd: y fp32 [B, C].  U3D_POOL_MAX: the rule of u3d_sparse_pool_fwd -- a strictly larger value replaces the held one,
 *     a NaN replaces a number, ties and later NaNs keep the lower row; arg int32 [B, C] = the winning row, -1 for an empty scene, whose
 *     y is +0.0.  U3D_POOL_AVG: the column sums of a scene in fp64, y = (float)(sum / n_b), one rounding to fp32; +0.0 for an empty
 *     scene; arg is not touched (may be NULL).  Two passes: partials per chunk of rows_per_chunk consecutive rows of one scene (16-byte
 *     loads, a group of lanes per row, the groups of a workgroup meet in LDS in a fixed tree), then one workgroup per scene over its
 *     chunks in ascending order: cut into consecutive runs, one per group of lanes, each added up chunk by chunk, the runs meeting in the
 *     same tree.  The summation order depends on (n_b, C) and the plan alone: results are bit-reproducible.
 *     ws: u3d_scene_pool_ws_bytes(n, B, C) = max_chunks * C * 8 bytes; nothing of it needs clearing.
 *   u3d_scene_pool_plan (host only): rows_per_chunk, max_chunks = ceil(n / rows_per_chunk) + B.  Either pointer may be NULL.
 *   u3d_scene_pool_bwd: gather form, dx[i, c] = dy[b(i), c] where arg[b(i), c] == i, else +0.0 (max); dx[i, c] = dy[b(i), c] * inv_b
 *     with inv_b = 1.0f / (float)n_b, each product rounded on its own (avg; arg may be NULL).  b(i) = the batch index of row i; a row
 *     whose batch index lies outside [0, B) gets +0.0.  Every element of dx is written exactly once: no atomics, no memset.
 *   Contract: 1 <= n < 2^31, 1 <= B <= 65535, C % 4 == 0, 4 <= C <= 512.  Errors, before any HIP call and with a u3d_last_error text:
 *   U3D_EINVAL for NULL pointers, n <= 0, B <= 0 and an unknown mode; U3D_EUNSUPPORTED for n >= 2^31, B > 65535 and other widths.  Empty
 *   tensors are the caller's business (no launch).  Outputs must not overlap the inputs.  Added entry points: U3D_ABI_VERSION is unchanged.
 * ===================================================================================== */
int u3d_scene_offsets(const int32_t* coords, int64_t n, int B, int32_t* offsets, int32_t* flag, u3d_stream_t stream);
int u3d_scene_topk_plan(int64_t n, int B, int* rows_per_block, int* blocks_per_scene);
int64_t u3d_scene_topk_ws_bytes(int64_t n, int B);
int u3d_scene_topk(const float* scores, const int32_t* coords, const int32_t* offsets, const int32_t* flag, const int32_t* k, int64_t n, int B,
                   int largest, uint8_t* mask, int32_t* kept, int32_t* pos, int32_t* result, void* ws, u3d_stream_t stream);
int u3d_scene_pool_plan(int64_t n, int B, int C, int* rows_per_chunk, int64_t* max_chunks);
int64_t u3d_scene_pool_ws_bytes(int64_t n, int B, int C);
int u3d_scene_pool_fwd(const float* x, const int32_t* offsets, int64_t n, int B, int C, int mode, float* y, int32_t* arg, void* ws,
                       u3d_stream_t stream);
int u3d_scene_pool_bwd(const float* dy, const int32_t* coords, const int32_t* offsets, const int32_t* arg, int64_t n, int B, int C, int mode,
                       float* dx, u3d_stream_t stream);

/* =====================================================================================
 * K13 self-attention core of nn.MultiheadAttention(256, 8, batch_first) per scene
 *     (unidet3d/encoder.py:19-20,36-37): softmax(Q K^T / sqrt(hd)) V over packed variable
 *     length scenes.  qkv [n_total, 3*H*hd] (the in_proj output), cu_seqlens int32 [B+1],
 *     out [n_total, H*hd], lse [H, n_total] (log-sum-exp, saved for backward).
 *     hd is 32 or 64 in all six entry points (any d_model / num_heads pair with that quotient); every other value returns
 *     U3D_EUNSUPPORTED ("head_dim <n> unsupported") before the first HIP call.  The native fp32 MFMA arm of the two fp32 entry
 *     points (u3d_fp32_math(0)) runs hd == 32 only and says so: the default three-plane mode runs 64.
 * ===================================================================================== */
int u3d_attn_varlen_fwd(const float* qkv, const int32_t* cu_seqlens, int B, int max_len, int64_t n_total,
                        int H, int hd, float scale, float* out, float* lse, double flops_hint,
                        u3d_stream_t stream);
int u3d_attn_varlen_bwd(const float* qkv, const float* out, const float* dout, const float* lse,
                        const int32_t* cu_seqlens, int B, int max_len, int64_t n_total, int H, int hd,
                        float scale, float* dqkv, float* delta_ws /*[H,n_total]*/, double flops_hint,
                        u3d_stream_t stream);
/* bf16-operand form of the two calls above (BASELINE configs[2]): identical arguments and results layout; Q/K/V/dO tiles and
 * the probabilities are rounded to bf16 for v_mfma_f32_16x16x32_bf16, softmax statistics and all accumulators stay fp32. */
int u3d_attn_varlen_fwd_bf16(const float* qkv, const int32_t* cu_seqlens, int B, int max_len, int64_t n_total, int H, int hd,
                             float scale, float* out, float* lse, double flops_hint, u3d_stream_t stream);
int u3d_attn_varlen_bwd_bf16(const float* qkv, const float* out, const float* dout, const float* lse, const int32_t* cu_seqlens,
                             int B, int max_len, int64_t n_total, int H, int hd, float scale, float* dqkv, float* delta_ws,
                             double flops_hint, u3d_stream_t stream);

/* bf16 TENSORS (K14b, csrc/gemm_b16.hip): qkv [n,3D], out [n,D], dout and dqkv are bf16 in HBM (one plane, no conversion while they
 * are staged; the score scale is applied to the scores), lse / delta_ws fp32 -- the tensors the reference's autocast hands to and
 * takes from nn.MultiheadAttention (tools/train.py:86-99). */
int u3d_attn_varlen_fwd_b16(const void* qkv, const int32_t* cu_seqlens, int B, int max_len, int64_t n_total, int H, int hd,
                            float scale, void* out, float* lse, double flops_hint, u3d_stream_t stream);
int u3d_attn_varlen_bwd_b16(const void* qkv, const void* out, const void* dout, const float* lse, const int32_t* cu_seqlens,
                            int B, int max_len, int64_t n_total, int H, int hd, float scale, void* dqkv, float* delta_ws,
                            double flops_hint, u3d_stream_t stream);

/* =====================================================================================
 * K13d  dropout of the decoder (unidet3d/encoder.py:19-22,38,55-61; csrc/dropout.h).  The mask is a stateless hash:
 *     keep(seed, offset, a, b, c)  <=>  hash32(seed, offset, a, b, c) >= floor(p 2^32).  Nothing is stored; a backward call
 *     regenerates the mask from the same (p, seed, offset).  The caller picks `offset` per (training step, site).
 *     Every entry point: p outside [0, 1) (NaN included) is U3D_EINVAL before the first HIP call.  Added entry points:
 *     U3D_ABI_VERSION is unchanged.
 *
 *     Attention: the six calls above with dropout on the softmax probabilities as in nn.MultiheadAttention --
 *     O = (P . M) V / (1 - p), lse from the undropped P -- with (a, b, c) = (head, packed query row, packed key row), rows counted in
 *     the packed [n_total, .] matrix.  p == 0 is the call above (the same kernels).  The native fp32 MFMA arm (u3d_fp32_math(0))
 *     is not built for p > 0: U3D_EUNSUPPORTED, the message names the mode that runs it.
 * ===================================================================================== */
int u3d_attn_varlen_fwd_drop(const float* qkv, const int32_t* cu_seqlens, int B, int max_len, int64_t n_total, int H, int hd,
                             float scale, float* out, float* lse, double flops_hint, u3d_stream_t stream, double p, uint64_t seed,
                             uint64_t offset);
int u3d_attn_varlen_bwd_drop(const float* qkv, const float* out, const float* dout, const float* lse, const int32_t* cu_seqlens,
                             int B, int max_len, int64_t n_total, int H, int hd, float scale, float* dqkv, float* delta_ws,
                             double flops_hint, u3d_stream_t stream, double p, uint64_t seed, uint64_t offset);
int u3d_attn_varlen_fwd_drop_bf16(const float* qkv, const int32_t* cu_seqlens, int B, int max_len, int64_t n_total, int H, int hd,
                                  float scale, float* out, float* lse, double flops_hint, u3d_stream_t stream, double p, uint64_t seed,
                                  uint64_t offset);
int u3d_attn_varlen_bwd_drop_bf16(const float* qkv, const float* out, const float* dout, const float* lse, const int32_t* cu_seqlens,
                                  int B, int max_len, int64_t n_total, int H, int hd, float scale, float* dqkv, float* delta_ws,
                                  double flops_hint, u3d_stream_t stream, double p, uint64_t seed, uint64_t offset);
int u3d_attn_varlen_fwd_drop_b16(const void* qkv, const int32_t* cu_seqlens, int B, int max_len, int64_t n_total, int H, int hd,
                                 float scale, void* out, float* lse, double flops_hint, u3d_stream_t stream, double p, uint64_t seed,
                                 uint64_t offset);
int u3d_attn_varlen_bwd_drop_b16(const void* qkv, const void* out, const void* dout, const float* lse, const int32_t* cu_seqlens,
                                 int B, int max_len, int64_t n_total, int H, int hd, float scale, void* dqkv, float* delta_ws,
                                 double flops_hint, u3d_stream_t stream, double p, uint64_t seed, uint64_t offset);
/* the mask itself, one byte per element (1 = kept): what the attention kernels apply for (p, seed, offset) over H heads of a packed
 * matrix of n_total rows, and what the elementwise kernels below apply to an [n, C] tensor ((a, b, c) = (0, row, column)) */
int u3d_dropout_mask_attn(double p, uint64_t seed, uint64_t offset, int H, int64_t n_total, uint8_t* mask /*[H][n_total][n_total]*/,
                          u3d_stream_t stream);
int u3d_dropout_mask_rows(double p, uint64_t seed, uint64_t offset, int64_t n, int C, uint8_t* mask /*[n][C]*/, u3d_stream_t stream);
/* elementwise dropout over [n, C]: y = x . M / (1 - p), formed in double and rounded once; backward is the same map on dy.  fp32
 * tensors (C % 4 == 0) and bf16 tensors (_b16, C % 8 == 0); 16-byte loads and stores, one launch. */
int u3d_dropout_fwd(const float* x, float* y, int64_t n, int C, double p, uint64_t seed, uint64_t offset, u3d_stream_t stream);
int u3d_dropout_bwd(const float* dy, float* dx, int64_t n, int C, double p, uint64_t seed, uint64_t offset, u3d_stream_t stream);
int u3d_dropout_fwd_b16(const void* x, void* y, int64_t n, int C, double p, uint64_t seed, uint64_t offset, u3d_stream_t stream);
int u3d_dropout_bwd_b16(const void* dy, void* dx, int64_t n, int C, double p, uint64_t seed, uint64_t offset, u3d_stream_t stream);

/* =====================================================================================
 * K14  dense fp32 GEMMs of the decoder's nn.Linear layers (unidet3d/encoder.py:19-21,55-61,138-140,
 *      153-155,163): forward C = A W^T + bias, input-gradient (the same call on the transposed weight),
 *      weight-gradient C = A^T B with the row reduction split over workgroups (ws, fixed-order sum).
 * ===================================================================================== */
int u3d_gemm_nt(const float* A /*[M,K]*/, const float* W /*[N,K]*/, const float* bias /*[N] or NULL*/, float* C /*[M,N]*/,
                int64_t M, int N, int K /* % 16 == 0 */, const void* w_planes, double flops_hint, u3d_stream_t stream);
/* OR-ed into `act` of u3d_linear_act / u3d_linear_dact / u3d_ffn_fwd: the MFMA operands are rounded to bf16 (round to nearest
 * even) on their way into LDS -- data stays fp32 in HBM, accumulation and epilogues stay fp32 (BASELINE configs[2]; the
 * reference trains with `--amp`, tools/train.py:86-99).  K must then be a multiple of 32. */
#define U3D_BF16_OPERANDS 16
/* Linear + activation in the GEMM epilogue (no separate elementwise kernel): Y = act(X W^T + bias), act: 0 none, 1 ReLU,
 * 2 GELU (erf form, unidet3d/encoder.py:58-59 `nn.GELU()`).  For GELU `pre` [M,N] receives X W^T + bias (kept for backward). */
int u3d_linear_act(const float* X /*[M,K]*/, const float* W /*[N,K]*/, const float* bias, int act, float* pre, float* Y /*[M,N]*/,
                   int64_t M, int N, int K, const void* w_planes, double flops_hint, u3d_stream_t stream);
/* input gradient THROUGH the activation: dX = (dY Wt^T) * act'(aux), Wt [N,K] = the next layer's weight transposed;
 * aux [M,N] = the ReLU output (act 1) or the GELU pre-activation (act 2). */
int u3d_linear_dact(const float* dY /*[M,K]*/, const float* Wt /*[N,K]*/, const float* aux, int act, float* dX /*[M,N]*/,
                    int64_t M, int N, int K, const void* w_planes, double flops_hint, u3d_stream_t stream);
/* C = A W^T + addend: a second gradient contribution folded into the GEMM that produces the first (flags: 0 or U3D_BF16_OPERANDS) */
int u3d_gemm_nt_add(const float* A /*[M,K]*/, const float* W /*[N,K]*/, const float* addend /*[M,N]*/, int flags, float* C, int64_t M,
                    int N, int K, const void* w_planes, double flops_hint, u3d_stream_t stream);
/* SURVEY.md 8(b) `ln_linear`: NQ = LayerNorm(X (+ RES)) (u3d_layer_norm_fwd: SUM receives X + RES, STATS the row statistics), then
 * Y = act(NQ W^T + bias) (u3d_linear_act) -- the head of the decoder (unidet3d/encoder.py:187-196: out_norm -> out_bboxes / outs_cls).
 * Two launches: the decoder is post-norm and NQ has further consumers, so the normalised rows are written in any case. */
int u3d_ln_linear(const float* X, const float* RES, const float* gamma, const float* beta, float eps, float* SUM, float* NQ, float* STATS,
                  const float* W /*[N,C]*/, const float* bias, int act, float* PRE, float* Y /*[M,N]*/, int64_t M, int C, int N,
                  const void* w_planes, double flops_hint, u3d_stream_t stream);
/* SURVEY.md 8(b) `ffn`: Z = act(X W1^T + b1) W2^T + b2 in two launches -- the FFN block (encoder.py:55-61, act 2), input_proj
 * (:138-140, act 1) and the class head (:153-155, act 1).  A [M,hid] receives the activation, H [M,hid] the GELU
 * pre-activation (NULL for ReLU); both are what the backward pass needs (u3d_linear_dact, u3d_gemm_tn). */
int u3d_ffn_fwd(const float* X, const float* W1 /*[hid,d_in]*/, const float* b1, const float* W2 /*[d_out,hid]*/, const float* b2,
                int act, float* H, float* A, float* Z /*[M,d_out]*/, int64_t M, int d_in, int hid, int d_out,
                const void* w1_planes, const void* w2_planes, double flops_hint, u3d_stream_t stream);
/* stand-alone erf-GELU passes (the unfused alternative to act = 2 above; n % 4 == 0): a = gelu(h); dh = da * gelu'(h) */
int u3d_gelu_fwd(const float* h, float* a, int64_t n, u3d_stream_t stream);
int u3d_gelu_bwd(const float* da, const float* h, float* dh, int64_t n, u3d_stream_t stream);
/* colsum_A (nullable, [N]): column sums of A -- the bias gradient of the Linear layer -- produced by the same pass */
int u3d_gemm_tn(const float* A /*[M,N]*/, const float* B /*[M,K]*/, float* C /*[N,K] = A^T B*/, float* colsum_A, int64_t M, int N, int K,
                void* ws, double flops_hint, u3d_stream_t stream);
/* bf16-operand form (BASELINE configs[2]): A and B are rounded to bf16 as they are staged, fp32 accumulation; colsum_A is
 * summed from the unrounded fp32 values.  Same workspace. */
int u3d_gemm_tn_bf16(const float* A, const float* B, float* C, float* colsum_A, int64_t M, int N, int K, void* ws, double flops_hint,
                     u3d_stream_t stream);
int64_t u3d_gemm_tn_ws_bytes(int64_t M, int N, int K);
int u3d_transpose(const float* in /*[R,C]*/, float* out /*[C,R]*/, int R, int C, u3d_stream_t stream);
/* All transposed copies of a step in one launch: desc int64 [n_desc][5] = {src ptr ([R][C] floats), dst ptr ([C][R]), R, C, first
 * block}; a matrix takes ceil(R/32) * ceil(C/32) blocks, total_blocks = their sum (descriptors in ascending first-block order). */
int u3d_transpose_batch(const void* desc, int n_desc, int64_t total_blocks, u3d_stream_t stream);
/* Pre-split W operands for the three-plane ("bf16x3") NT products.  u3d_weight_planes_batch: desc int64 [n_desc][4] = {src ptr (fp32,
 * n8 * 8 values), dst ptr (bf16 [3][n8 * 8]: the three exact planes of every value, 8-element groups split exactly as the GEMM
 * kernels split them in flight), n8, first block}; a matrix takes ceil(n8 / 256) blocks; one launch for every weight (and transposed
 * copy) of a training step.  The `w_planes` argument of the NT entry points above (u3d_gemm_nt, u3d_linear_act, u3d_linear_dact,
 * u3d_gemm_nt_add, u3d_ln_linear; u3d_ffn_fwd takes one for W1 and one for W2) is such a matrix's planes ([3][N][K] bf16, same N, K
 * as the fp32 W of that call, which must still be passed) or NULL: the call reads its W operand from them when it runs the
 * three-plane kernel and ignores them otherwise (bf16 operands, the native fp32 math mode, K % 32 != 0).  Results are bit-identical
 * with and without. */
int u3d_weight_planes_batch(const void* desc, int n_desc, int64_t total_blocks, u3d_stream_t stream);

/* ---- K14b: the same Linear layers with bf16 ACTIVATIONS in HBM (csrc/gemm_b16.hip; BASELINE configs[2] -- the reference's `--amp`
 * autocasts the Linear / MultiheadAttention activations, tools/train.py:86-99 around unidet3d/encoder.py:19-21,55-61,138-163).
 * `flags` says which tensors ARE bf16 (row-major, 2 bytes an element); everything else is fp32.  Products run on bf16 MFMAs with
 * fp32 accumulation exactly as under U3D_BF16_OPERANDS (an fp32 operand is rounded to nearest even while it is staged), so a bf16
 * tensor that holds the RNE rounding of an fp32 one gives bit-identical products. */
#define U3D_A_BF16 1   /* the first streamed operand (A) */
#define U3D_B_BF16 2   /* u3d_gemm_tn_b16: the second streamed operand (B) */
#define U3D_C_BF16 4   /* u3d_gemm_nt_b16: the result C -- and `aux` of epi 3 */
/* C[M,N] = epi(A[M,K] W[N,K]^T): epi 0: + bias | 1: relu(+ bias) | 3: aux > 0 ? . : 0 (aux [M,N] = the ReLU output, C's dtype) |
 * 5: + aux (aux and C fp32).  W and bias are fp32.  K % 32 == 0; a bf16 C needs an even N. */
int u3d_gemm_nt_b16(const void* A, const float* W, const float* bias, int epi, const void* aux, void* C, int flags, int64_t M, int N, int K,
                    double flops_hint, u3d_stream_t stream);
/* C[N,K] = A[M,N]^T B[M,K] (fp32), colsum_A (nullable, [N]) = column sums of A; flags: U3D_A_BF16 | U3D_B_BF16.  N (K) % 8 == 0 for a
 * bf16 A (B), % 4 otherwise.  ws: u3d_gemm_tn_b16_ws_bytes.  Fixed-order reduction over the row splits (deterministic). */
int u3d_gemm_tn_b16(const void* A, const void* B, float* C, float* colsum_A, int flags, int64_t M, int N, int K, void* ws, double flops_hint,
                    u3d_stream_t stream);
int64_t u3d_gemm_tn_b16_ws_bytes(int64_t M, int N, int K);
/* erf GELU between bf16 tensors (n % 8 == 0): a = gelu(h); dh = da * gelu'(h) */
int u3d_gelu_fwd_b16(const void* h, void* a, int64_t n, u3d_stream_t stream);
int u3d_gelu_bwd_b16(const void* da, const void* h, void* dh, int64_t n, u3d_stream_t stream);

/* ---- what a GEMM launch with the same sizes WOULD do (pure host functions: no GPU, no HIP call; like u3d_spconv_plan).  Each query
 * calls the very function its launch path takes the decision from, so it reports the current fp32 math mode (u3d_fp32_math) and the
 * environment overrides (U3D_NT_TILE, U3D_NT16_TILE, U3D_TN_WGS, U3D_TN16_WGS, U3D_TN_X3) as well, and returns the launch's own
 * status for sizes the launch refuses (U3D_EINVAL: a size <= 0, an unknown epi / flag; U3D_EUNSUPPORTED with a message: K no multiple
 * of 16 / 32, TN with N or K no multiple of 4 / 8, an odd N or epi 5 with a bf16 C, 32-bit offsets).  Output pointers may be NULL.
 * Kernel families: */
#define U3D_GEMM_NATIVE 0 /* v_mfma_f32_32x32x2_f32 on fp32 operands: gemm_nt_k, gemm_tn_k */
#define U3D_GEMM_X3 1     /* three bf16 planes per fp32 operand: gemm_nt_x3_k (W split in flight or passed as w_planes), gemm_tn_x3_k */
#define U3D_GEMM_B16 2    /* operands rounded to bf16: gemm_nt_b16_k; gemm_tn_bf16_k (u3d_gemm_tn_bf16), gemm_tn_b16_k (u3d_gemm_tn_b16) */
/* u3d_gemm_nt / u3d_linear_act / u3d_linear_dact / u3d_gemm_nt_add / u3d_ffn_fwd (one query per product); flags: 0 or
 * U3D_BF16_OPERANDS.  tile_m x tile_n: rows x columns of C per workgroup (128 x 128, 128 x 64 or 64 x 64). */
int u3d_gemm_nt_plan(int64_t M, int N, int K, int flags, int* kernel, int* tile_m, int* tile_n);
/* u3d_gemm_nt_b16 (always U3D_GEMM_B16); epi and flags as there */
int u3d_gemm_nt_b16_plan(int64_t M, int N, int K, int epi, int flags, int* tile_m, int* tile_n);
/* u3d_gemm_tn (bf16_operands = 0) / u3d_gemm_tn_bf16 (1).  tile_n x tile_k: rows x columns of C[N,K] per workgroup; the M rows are
 * cut into `splits` pieces of rows_per_split rows (whole trips of the kernel: the last piece may be ragged, and pieces that begin at
 * or past row M are empty -- they still write a zero partial, which the fixed-order reduce sums). */
int u3d_gemm_tn_plan(int64_t M, int N, int K, int bf16_operands, int* kernel, int* tile_n, int* tile_k, int* splits, int64_t* rows_per_split);
/* u3d_gemm_tn_b16 (always U3D_GEMM_B16, 128 x 128 tiles); flags as there */
int u3d_gemm_tn_b16_plan(int64_t M, int N, int K, int flags, int* tile_n, int* tile_k, int* splits, int64_t* rows_per_split);

/* =====================================================================================
 * K15 LayerNorm of the decoder (unidet3d/encoder.py:21,38-40,61,78-79,140,167) with the preceding residual add fused in.
 *      forward: s = x (+ res), y = (s - mean) * rstd * gamma + beta; sum_out receives s when res != NULL (the tensor
 *      the backward needs), stats [M][2] = (mean, rstd).  backward: dx (= gradient of both x and res), dgamma, dbeta
 *      (per-workgroup partials in ws, fixed-order sum).  C % 4 == 0, C <= 1024.
 * ===================================================================================== */
int u3d_layer_norm_fwd(const float* x, const float* res, const float* gamma, const float* beta, int64_t M, int C, float eps,
                       float* sum_out, float* y, float* stats, u3d_stream_t stream);
int u3d_layer_norm_bwd(const float* s, const float* dy, const float* gamma, const float* stats, int64_t M, int C, float* dx,
                       float* dgamma, float* dbeta, void* ws, u3d_stream_t stream);
/* the same passes, additionally writing y (dx) rounded to bf16 into y16 (dx16) [M,C] -- the copy the next GEMM streams (K14b);
 * y16 / dx16 NULL = the calls above */
int u3d_layer_norm_fwd_b16(const float* x, const float* res, const float* gamma, const float* beta, int64_t M, int C, float eps,
                           float* sum_out, float* y, void* y16, float* stats, u3d_stream_t stream);
int u3d_layer_norm_bwd_b16(const float* s, const float* dy, const float* gamma, const float* stats, int64_t M, int C, float* dx, void* dx16,
                           float* dgamma, float* dbeta, void* ws, u3d_stream_t stream);
/* the backward pass of a LayerNorm whose RESULT had up to three consumers (the decoder: the next Linear, the residual into the next
 * LayerNorm, the prediction head -- unidet3d/encoder.py:21,38-40,221-239): the incoming gradient is dy + dy2 + dy3 (dy2 / dy3 nullable),
 * summed as the rows are read instead of by two elementwise passes in front of this call; otherwise u3d_layer_norm_bwd_b16 */
int u3d_layer_norm_bwd_sum(const float* s, const float* dy, const float* dy2, const float* dy3, const float* gamma, const float* stats,
                           int64_t M, int C, float* dx, void* dx16, float* dgamma, float* dbeta, void* ws, u3d_stream_t stream);
int64_t u3d_layer_norm_ws_bytes(int64_t M, int C);

/* ---- inference post-processing of one scene ------------------------------------------------
 * u3d_nms_bev: replaces UniDet3D._single_scene_multiclass_nms with fast_nms=True (unidet3d/unidet3d.py:595-650, which
 * calls mmcv.ops.nms3d_normal per class: greedy suppression by the IoU of the (x, y, dx, dy) rectangles).  boxes [n][6]
 * = (cx, cy, cz, dx, dy, dz) and labels [n] must be ordered by (label ascending, score descending) -- the order the
 * reference visits them in; keep[n] receives 1 for surviving boxes.  n <= 4400 (one workgroup holds the boxes in LDS; the configs use top-k = 1000). */
int u3d_nms_bev(const float* boxes, const int32_t* labels, int n, float iou_thr, uint8_t* keep, u3d_stream_t stream);
/* fast_nms=False branch (unidet3d.py:634-636): mmdet3d aligned_3d_nms on corner boxes (x1,y1,z1,x2,y2,z2) = _bbox_to_loss(boxes);
 * same ordering contract; a box survives only while its 3-D IoU with every kept box of its class is <= iou_thr. */
int u3d_nms_aligned3d(const float* corners, const int32_t* labels, int n, float iou_thr, uint8_t* keep, u3d_stream_t stream);
/* rotated boxes (unidet3d.py:625-626, mmcv.ops.nms3d): boxes [n][7] = (cx, cy, cz, dx, dy, dz, heading); suppression by the BEV IoU
 * of the rotated rectangles; same ordering contract, n <= 3600. */
int u3d_nms_rotated(const float* boxes, const int32_t* labels, int n, float iou_thr, uint8_t* keep, u3d_stream_t stream);
/* u3d_trim_boxes: replaces UniDet3D.trim_bboxes_by_superpoints + get_face_distances (unidet3d/unidet3d.py:540-593, :652-677)
 * points: rows of >= 3 floats with leading dimension pt_ld; (sp_list, sp_offsets[S+1]): CSR of point rows per superpoint
 * (u3d_csr_build).  boxes [nb][box_dim], box_dim = 6 (cx, cy, cz, dx, dy, dz) or 7 (+ heading: the point shift is rotated by
 * -heading about z before the six face tests, as get_face_distances does).  minmax [nb][6] receives (min xyz, max xyz) of the points selected for each box
 * (+inf / -inf when none, as in the reference); centre = (max+min)/2 and size = max-min are left to the caller. */
int u3d_trim_boxes(const float* points, int64_t pt_ld, const int32_t* sp_list, const int32_t* sp_offsets, int S,
                   const float* boxes, int nb, int box_dim, float low_thr, float up_thr, float* minmax, u3d_stream_t stream);

/* ---- inference post-processing of a whole batch: one chain of launches, no host read in between ---------------------------
 * The batched form of softmax -> top-k -> class-wise NMS -> superpoint trimming (UniDet3D.predict_by_feat for every scene of a
 * batch, each scene with its own dataset's settings).  Per-scene settings are two small device tables:
 *   meta  int32 [B][U3D_PP_META] = {n queries, C classes, ld (row stride of the probability matrix, elements; >= C),
 *                                   topk, box_dim (6 | 7), NMS mode (0 BEV IoU = nms3d_normal, 1 3-D IoU of the corner boxes =
 *                                   aligned_3d_nms, 2 rotated BEV IoU = nms3d; 7-column boxes must use 2), trim (0 | 1), 0}
 *   fmeta float [B][U3D_PP_FMETA] = {score_thr, iou_thr, low_sp_thr, up_sp_thr}
 * K is the per-scene stride of every [B][K] array: the entries of scene b start at row b * K.  K <= 3600 (a class segment of
 * rotated boxes must fit one workgroup's LDS; callers fall back to the per-scene entry points above it).  n * C < 2^31. */
#define U3D_PP_META 8
#define U3D_PP_FMETA 4
/* top k of each scene's n x C probabilities, read in place: element (q, c) of scene b at ((const float*)prob_ptrs[b])[q * ld + c]
 * (the first C columns of softmax(cls_preds), without copying [:, :-1]).  Probabilities must be >= 0 (their bit patterns order
 * as uint32).  score / label (flat % C) / query (flat / C) [B][K] in descending score, ties by ascending flat index
 * (np.argsort(-x, kind='stable')); count [B] = min(topk, K, n * C) entries written per scene. */
int u3d_topk_segmented(const uint64_t* prob_ptrs, const int32_t* meta, int B, int K, float* score, int32_t* label, int32_t* query,
                       int32_t* count, u3d_stream_t stream);
/* class-wise greedy NMS of the top-k candidates of every scene.  Per scene: candidates with score <= score_thr are dropped, the
 * rest are stably ordered by label (torch.sort(labels, stable=True) of the score-sorted list): order [B][K] = candidate rank r,
 * n_order [B] = how many; boxes_ord [B][K][7] = the candidates' boxes (row query[r] of the scene's [n][box_dim] box matrix at
 * box_ptrs[b]) in that order, heading 0 for 6-column boxes; keep [B][K] = 1 for the survivors of the greedy suppression inside
 * each (scene, class) segment -- the same arithmetic, and so the same flags, as u3d_nms_bev / u3d_nms_aligned3d /
 * u3d_nms_rotated on the scene's ordered list.  max_classes >= every C.  ws: u3d_nms_batched_ws_bytes(B, max_classes). */
int u3d_nms_batched(const uint64_t* box_ptrs, const int32_t* meta, const float* fmeta, int B, int K, int max_classes, const float* score,
                    const int32_t* label, const int32_t* query, const int32_t* count, int32_t* order, int32_t* n_order, uint8_t* keep,
                    float* boxes_ord, void* ws, u3d_stream_t stream);
int64_t u3d_nms_batched_ws_bytes(int B, int max_classes);
/* stable compaction of the keep flags: the survivors of scene b in the reference's output order (label asc, score desc) at rows
 * b * K .. b * K + out_count[b] of out_boxes [B][K][7], out_scores [B][K], out_labels int64 [B][K]; yaw [B] = 1 when a survivor
 * has a non-zero (or NaN) heading; minmax [B][K][6] is set to (+inf, -inf) for the survivors of trimmed scenes. */
int u3d_nms_compact(const int32_t* meta, int B, int K, const float* score, const int32_t* label, const int32_t* order, const int32_t* n_order,
                    const uint8_t* keep, const float* boxes_ord, float* out_boxes, float* out_scores, int64_t* out_labels, int32_t* out_count,
                    int32_t* yaw, float* minmax, u3d_stream_t stream);
/* superpoint trimming of the boxes of every scene with trim = 1 (u3d_trim_boxes per scene): (sp_list, sp_offsets [S+1]) is the
 * batch-global CSR of point rows per superpoint, sp_scene int32 [B+1] the first superpoint of each scene; a superpoint is paired
 * with its own scene's out_count[b] boxes only, which are rotated by their heading when yaw[b] != 0 and taken as yaw-free
 * otherwise.  minmax as u3d_nms_compact left it; boxes [B][K][7] (u3d_nms_compact's out_boxes): columns 0..5 of the trimmed
 * scenes' rows are replaced by (centre, size) = ((max + min) / 2, max - min) of the selected points. */
int u3d_trim_boxes_batched(const float* points, int64_t pt_ld, const int32_t* sp_list, const int32_t* sp_offsets, const int32_t* sp_scene,
                           int B, int S, const int32_t* meta, const float* fmeta, int K, const int32_t* count, const int32_t* yaw,
                           float* minmax, float* boxes, u3d_stream_t stream);

/* =====================================================================================
 * R12  matcher + losses of a batch on the device: forward value AND gradients in five launches
 *      (unidet3d/criterion.py:44-178, :200-320; unidet3d/axis_aligned_iou_loss.py:14-53; unidet3d/rotated_iou_loss.py:14-82).
 *      Single-dataset AND mixed batches of the joint config: every scene has its own dataset (class columns, top-k, weight)
 *      and box parametrisation (6-dof axis-aligned, or 7-dof with a heading -> rotated DIoU in the matcher cost and the loss).
 *  cls [L][n_tot][CU]: logits of the L decoder heads, scenes packed, CU columns per row; box [L][n_tot][BD], BD = 6 (centre, size)
 *  or 7 (+ heading; a yaw-free scene of a 7-column batch ignores its heading column and receives a zero gradient there);
 *  cu int32 [B+1] first query of a scene; gt_off int32 [B+1] first GT of a scene; gt_labels int64 [G] (index into the scene's class
 *  list); gt_boxes [G][BD]; qmask uint8: scene b's [g_b][n_b] query mask at qm_off[b] (int64 [B+1] = prefix sums of n_b g_b,
 *  P = qm_off[B]); scene_meta int32 [B][4] = {classes + 1 of the scene's dataset (the last one is "no object"), top-k,
 *  1 if the scene's boxes carry a heading, offset of the scene's class-column list in cidx}; scene_w float [B] dataset weight;
 *  cidx int32 (nullable): concatenated class-column lists (logit of class c of scene b = cls[..][cidx[off_b + c]]); NULL = the
 *  scene's classes are columns 0 .. C1-1.  max_gt = max g_b, any value: the matched set of a (layer, query) is kept in
 *  ceil(max_gt / 64) 64-bit words, and a batch with max_gt > 64 computes its cost matrix with one thread per (layer, query, GT)
 *  entry instead of one per (layer, query) (one more launch).  With max_gt <= 64 the launches and the arithmetic are what they
 *  were with the one-word mask, bit for bit.  What bounds a scene is 32-bit indexing: n_tot, G, L * G and
 *  min(P, n_tot * max_gt) -- an upper bound of every scene's n_b * g_b -- must fit an int; otherwise U3D_EUNSUPPORTED before
 *  anything is launched.  min_query_slack = min over scenes with g_b > 0 of n_b - (topk_b + 1) (must be >= 0, as torch.topk
 *  requires in the reference).
 *  loss [1] = sum over layers of lw_cls * mean_b(w_b CE_b) + lw_box * mean over scenes with matches (w_b DIoU_b);
 *  dcls [L][n_tot][CU] / dbox [L][n_tot][BD] receive d loss / d cls (zero in columns outside the scene's class list), d loss / d box.
 *  ws: u3d_criterion_ws_bytes_gt for the same max_gt (u3d_criterion_ws_bytes: the size for max_gt <= 64; the _gt query is an
 *  ADDED entry point and no argument list moved, so U3D_ABI_VERSION is unchanged).  NOTE for callers of the C interface: with
 *  max_gt > 64 the entry point used to refuse; it now runs and needs the larger workspace, and it cannot see how ws was sized -- a
 *  workspace sized by the five-argument query and used with max_gt > 64 is overrun.  Size ws with the _gt query whenever max_gt can
 *  exceed 64.  The five-argument query itself returns L * n_tot * 8 bytes (rounded up to 64) more than it did for the same
 *  arguments: the block of the log-sum-exp pre-pass is always part of the layout.
 *  Errors: U3D_EINVAL with a message for max_gt outside [0, G]; U3D_EUNSUPPORTED with a message for L > 65535 and for the 32-bit
 *  bound above -- that message names the bound and the batch totals, not the scene: the scene sizes are device arrays here (the
 *  Python host, which knows them, names the scene).
 *  Environment: U3D_CRITERION_COST=query | pair (read once per process) forces the per-query or the per-entry cost kernel
 *  whatever max_gt is, for A/B timing (tools/criterion_time.py); both evaluate the same expression per entry.
 *  Unset: per-entry iff max_gt > 64.
 *  Layout: cost [L][P], logz [L][n_tot], kth [L][G], match words uint64 [L][n_tot][W], W = max(1, ceil(max_gt / 64)) (GT j of the
 *  query's scene = bit j & 63 of word j >> 6), statistics; every block starts on a multiple of 64 bytes. */
int u3d_criterion_packed(const float* cls, const float* box, const int32_t* cu, const int32_t* gt_off, const int64_t* gt_labels,
                         const float* gt_boxes, const uint8_t* qmask, const int64_t* qm_off, const int32_t* scene_meta,
                         const float* scene_w, const int32_t* cidx, int L, int B, int64_t n_tot, int CU, int BD, int64_t G, int64_t P,
                         int max_gt, int min_query_slack, float w_cls, float w_box, float non_obj_w, float lw_cls, float lw_box,
                         float* loss, float* dcls, float* dbox, void* ws, u3d_stream_t stream);
int64_t u3d_criterion_ws_bytes(int L, int B, int64_t n_tot, int64_t G, int64_t P);
int64_t u3d_criterion_ws_bytes_gt(int L, int B, int64_t n_tot, int64_t G, int64_t P, int max_gt);
/* box decode of a yaw-free head in one pass each way: PredBBox's exp of the six face distances + _bbox_pred_to_bbox
 * (unidet3d/encoder.py:99-111, :241-271): raw [M][8] (Linear output), centers [M][3] -> box [M][6] (centre, size);
 * backward: draw [M][8] from dbox [M][6] (the angle columns receive 0). */
int u3d_box_decode_fwd(const float* raw, const float* centers, int64_t M, float* box, u3d_stream_t stream);
int u3d_box_decode_bwd(const float* raw, const float* dbox, int64_t M, float* draw, u3d_stream_t stream);
/* the same for a head with a heading / a mixed batch (encoder.py:241-283 incl. the rotated branch): box [M][7] = (centre, w, l, size_z,
 * alpha) on rows with a heading -- yaw_rows[i] != 0, or every row when yaw_rows == NULL -- and (centre, size, 0) on the others, whose
 * raw heading columns get a zero gradient (the reference never evaluates them for scenes of yaw-free datasets, encoder.py:186-199). */
int u3d_box_decode7_fwd(const float* raw, const float* centers, const uint8_t* yaw_rows, int64_t M, float* box, u3d_stream_t stream);
int u3d_box_decode7_bwd(const float* raw, const float* dbox, const uint8_t* yaw_rows, int64_t M, float* draw, u3d_stream_t stream);

/* =====================================================================================
 * R13  training-input augmentation of a whole ragged batch on the device (csrc/augment.hip): the steps of the reference's ScanNet /
 *      S3DIS train pipelines after file loading -- PointSample_, RandomFlip3D, GlobalRotScaleTrans, NormalizePointsColor_
 *      (unidet3d/loading.py:71-107), ElasticTransfrom, PointDetClassMappingScanNet / S3DIS (unidet3d/transforms_3d.py:12-295).
 *  The batch is the concatenated per-point arrays plus pt_offsets int64 [B+1]; every entry point covers all scenes in a fixed
 *  number of launches.  Source arrays (a device-resident scene cache of src_rows rows) are addressed through src int64 [B][2] =
 *  (first row, row count) of each scene and an optional gather int64 [n]: batch point i of scene b reads source row
 *  first_b + gather[i] % count_b (a draw below the count is taken as it is), or first_b + (i - pt_offsets[b]) when gather is NULL.
 *  Zero points / zero scenes / an empty scene inside a batch are valid (nothing is launched for them) or U3D_EINVAL.
 * ===================================================================================== */
/* points [n][6] = (affine_b (x, y, z), colour): x' = ((a00 x + a01 y) + a02 z) + a03 in fp32 in this order, affine float [B][3][4];
 * colour c' = (c - mean) / std, fp32 subtract then fp32 divide, each only when its host pointer (3 floats) is non-NULL;
 * coords (nullable) [n][3] = x' / voxel_size, IEEE fp32 division (what ElasticTransfrom.transform starts from). */
int u3d_aug_points(const float* src_points, int64_t src_rows, const int64_t* gather, const int64_t* src, const int64_t* pt_offsets, int B,
                   int64_t n, const float* affine, const float* color_mean_host, const float* color_std_host, float voxel_size,
                   float* points, float* coords, u3d_stream_t stream);
/* extent [B][3] = max |coord| per scene and axis (0 for an empty scene), exact; coords [n][3]. */
int u3d_aug_extent_f32(const float* coords, const int64_t* pt_offsets, int B, int64_t max_pts_per_scene, float* extent, u3d_stream_t stream);
int u3d_aug_extent_f64(const double* coords, const int64_t* pt_offsets, int B, int64_t max_pts_per_scene, double* extent, u3d_stream_t stream);
/* the six sweeps of transforms._box_blur3 (axes 0,1,2,0,1,2, zero padding, (a/3' + b/3') + c/3' with 3' = fp32(1/3) as products)
 * over the noise grids of one elastic pass: noise holds scene b's [3][d0][d1][d2] floats at 3 grid_offsets[b] (grid_offsets int64
 * [B+1] in cells, dims int32 [B][3]; a scene without a pass has zero cells).  grids receives them cell-major: 4 floats per cell
 * (channel 0, 1, 2, unused) at cell grid_offsets[b] + (i0 d1 + i1) d2 + i2.  Six launches.  ws: u3d_aug_noise_blur_ws_bytes. */
int u3d_aug_noise_blur(const float* noise, const int32_t* dims, const int64_t* grid_offsets, int B, int64_t total_cells, float* grids,
                       void* ws, u3d_stream_t stream);
int64_t u3d_aug_noise_blur_ws_bytes(int64_t total_cells);
/* one elastic pass: out = x + trilinear(grids)(x) * mag per point in fp64 (transforms.trilinear_lookup: t = (x + (b-1) gran) / (2 gran),
 * i0 = clip(floor(t), 0, b-2), 0 outside [0, b-1], eight corners in (dx, dy, dz) order); coords_in fp32 or fp64 [n][3] (in_f64),
 * coords_out likewise (out_f64).  Scenes with gate[b] == 0 pass x through unchanged. */
int u3d_aug_elastic(const void* coords_in, int in_f64, void* coords_out, int out_f64, const int64_t* pt_offsets, int B, int64_t n,
                    const float* grids, const int64_t* grid_offsets, const int32_t* dims, const uint8_t* gate, double gran, double mag,
                    u3d_stream_t stream);
/* np.unique(ids, return_inverse=True)[1] per scene for ids in [-1, max_id]: scene b owns table_offsets[b+1] - table_offsets[b] =
 * max_id_b + 2 table entries (table_offsets int64 [B+1]); an id outside that range counts as -1.  keep_negative: -1 stays -1 and
 * the other ids become 0..k-1.  sem (nullable, a source array like ids): sem_out [n] (nullable) receives the gathered labels, and
 * points whose label l has sem_drop[l] != 0 (uint8 [n_sem_drop], nullable) take id -1 first.  counts int32 [B] = distinct ids that
 * received a rank; first (nullable) int64 [table_entries]: batch row of the first occurrence of new id r of scene b at
 * table_offsets[b] + r (np.unique's return_index), 0 past the count.  ws: u3d_relabel_ids_ws_bytes. */
int u3d_relabel_ids(const int64_t* ids, int64_t src_rows, const int64_t* gather, const int64_t* src, const int64_t* pt_offsets, int B, int64_t n,
                    const int64_t* table_offsets, int64_t table_entries, int keep_negative, const int64_t* sem, const uint8_t* sem_drop,
                    int n_sem_drop, int64_t* new_ids, int64_t* sem_out, int32_t* counts, int64_t* first, void* ws, u3d_stream_t stream);
int64_t u3d_relabel_ids_ws_bytes(int64_t table_entries);
/* ids[i] = table[table_offsets[b] + ids[i]] in place for ids inside the scene's table, -1 otherwise (PointDetClassMappingS3DIS's remap). */
int u3d_aug_remap_ids(int64_t* ids, const int64_t* pt_offsets, int B, int64_t n, const int64_t* table, const int64_t* table_offsets,
                      u3d_stream_t stream);
/* transforms._sp_masks of every scene: masks (uint8 0 / 1), scene b's [n_inst_b][S_b] matrix at mask_offsets[b] (int64 [B+1]),
 * S_b = sp_offsets[b+1] - sp_offsets[b]; entry (j, s) = 2 hits[j][s] > cnt[s].  inst [n] in batch order; sp [n] in batch order, or a
 * source array read through sp_src (the `src` table) when that is non-NULL.  ws: u3d_aug_sp_masks_ws_bytes. */
int u3d_aug_sp_masks(const int64_t* inst, const int64_t* sp, const int64_t* sp_src, int64_t src_rows, const int64_t* pt_offsets, int B, int64_t n,
                     const int32_t* n_inst, const int64_t* sp_offsets, const int64_t* mask_offsets, int64_t mask_entries, int64_t n_superpoints,
                     uint8_t* masks, void* ws, u3d_stream_t stream);
int64_t u3d_aug_sp_masks_ws_bytes(int64_t mask_entries, int64_t n_superpoints);
/* u3d_aug_points with DenormalizePointsColor (unidet3d/loading.py:123-143) in front of the normalisation:
 * c' = (((c * dstd) + dmean) - mean) / std in fp32 in this order, every step only when its host pointer (3 floats) is non-NULL.
 * With both denorm pointers NULL the result equals u3d_aug_points' bit for bit. */
int u3d_aug_points_dn(const float* src_points, int64_t src_rows, const int64_t* gather, const int64_t* src, const int64_t* pt_offsets, int B,
                      int64_t n, const float* affine, const float* color_mean_host, const float* color_std_host,
                      const float* denorm_mean_host, const float* denorm_std_host, float voxel_size, float* points, float* coords,
                      u3d_stream_t stream);
/* the ground-truth boxes of a box-annotated batch through the scenes' flip / rotation / scale / translation, one thread per box:
 * src_boxes [src_rows][7] = (gravity centre, size, yaw) rows of the scene cache, box_src int64 [B][2] = (first row, row count) per
 * scene, box_offsets int64 [B+1], boxes [n][7].  Centre: the point map's fp32 expression with affine [B][3][4]; size * fp32(scale);
 * yaw in fp64 -- flip_h: pi - yaw, flip_v: -yaw, then + angle -- rounded once to fp32, no period wrapping; scalars double [B][4] =
 * (flip_h, flip_v, angle, scale); scenes with with_yaw[b] == 0 (uint8 [B]) get yaw 0. */
int u3d_aug_boxes(const float* src_boxes, int64_t src_rows, const int64_t* box_src, const int64_t* box_offsets, int B, int64_t n,
                  const float* affine, const double* scalars, const uint8_t* with_yaw, float* boxes, u3d_stream_t stream);

/* =====================================================================================
 * R14  distance targets of every scene of a batch (csrc/targets.hip; unidet3d/unidet3d.py:371-409 get_targets): scene b owns the
 *      superpoint centres centers[sp_offsets[b] .. sp_offsets[b+1]) ([n_sp][3] fp32) and the boxes box_offsets[b] .. box_offsets[b+1]
 *      of box_centers (gravity centres, row g at box_centers + g box_ld, box_ld >= 3 floats, n_boxes rows).  masks (uint8 0 / 1)
 *      receives scene b's [G_b][S_b] matrix row-major at mask_offsets[b] (int64 [B+1], mask_entries in all), zeros included:
 *      d = ((cx-px)^2 + (cy-py)^2) + (cz-pz)^2 in fp32; kth[g] = the min(topk+1, S_b)-th smallest d of box g; superpoint s goes to
 *      the box with the smallest d among those with d < kth[g] (strictly; lowest index on ties; none at d >= 1e8).  Scenes without
 *      boxes or superpoints are valid.  max_boxes / max_sp: the largest G_b / S_b (they size the two grids).  topk + 1 <= 16, else
 *      U3D_EUNSUPPORTED.  Two launches, no atomics.  ws: u3d_targets_by_distance_ws_bytes(n_boxes).
 * ===================================================================================== */
int u3d_targets_by_distance(const float* centers, int64_t n_sp, const int64_t* sp_offsets, const float* box_centers, int64_t box_ld,
                            int64_t n_boxes, const int64_t* box_offsets, const int64_t* mask_offsets, int64_t mask_entries, int B,
                            int64_t max_boxes, int64_t max_sp, int topk, uint8_t* masks, void* ws, u3d_stream_t stream);
int64_t u3d_targets_by_distance_ws_bytes(int64_t n_boxes);

/* =====================================================================================
 * R15  optimizer tail of a training step (csrc/optim.hip): global gradient norm, clipping and AdamW with decoupled weight decay
 *      over every parameter tensor in two launches -- torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW of the reference's
 *      optim_wrapper (configs/unidet3d_1xb8_scannet.py:710-715).  Both entry points read one device table `rows`, int64 [n_rows][8]:
 *        0 parameter pointer (fp32)        1 gradient pointer (fp32; 0: the parameter is skipped this step)
 *        2 offset of the row's moments in exp_avg / exp_avg_sq, in floats, a multiple of 4      3 numel
 *        4 lr, 5 weight decay (the bit patterns of two doubles)
 *        6 global steps the parameter has missed: its own step count, which the bias corrections use, is step - rows[i][6] >= 1
 *        7 first block: row i owns blocks [rows[i][7], rows[i][7] + ceil(numel / U3D_OPTIM_CHUNK)), rows ascending, total_blocks in all
 *      Block b serves the last row whose first block is <= b.  A row whose parameter and gradient pointers are 16-byte aligned moves
 *      dwordx4, any other row dwords, with the same arithmetic per element: results do not depend on alignment.  No atomics, every
 *      sum in a fixed order: results are bit-reproducible.  Gradients are only read (p.grad stays unclipped).
 * ===================================================================================== */
#define U3D_OPTIM_CHUNK 4096     /* elements of a row per block */
#define U3D_OPTIM_PARTIALS 512   /* fp64 partial sums of squares in the workspace */
int u3d_optim_chunk(void);       /* U3D_OPTIM_CHUNK of the library that was loaded */
int64_t u3d_optim_ws_bytes(void);
/* ws[j] (double) = sum over the gradient elements of chunk run j of g^2, squares and sums in fp64.  One launch. */
int u3d_optim_grad_sumsq(const void* rows, int n_rows, int64_t total_blocks, void* ws, u3d_stream_t stream);
/* One launch.  max_norm > 0: norm = sqrt(sum of ws) rounded to fp32 is stored to *total_norm (one thread) and every gradient is
 * read as g * min(1, max_norm / (norm + 1e-6)) (fp32; ws from u3d_optim_grad_sumsq on the same table and stream);
 * max_norm <= 0: no clipping, ws and total_norm are not touched.  Then, per element, in the order and mixed precision of torch's fused
 * AdamW (doubles for the hyper-parameters, one rounding to fp32 per assignment), with t the row's own step count:
 *   p -= lr wd p;  m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g g;
 *   p -= (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps).
 * step: the global step count INCLUDING this step (>= 1).  U3D_EINVAL, before any launch: rows NULL, n_rows or total_blocks
 * negative, a moment buffer that is NULL or not 16-byte aligned, step < 1, clipping without ws / total_norm. */
int u3d_optim_adamw(const void* rows, int n_rows, int64_t total_blocks, float* exp_avg, float* exp_avg_sq, double beta1, double beta2,
                    double eps, float max_norm, int64_t step, const void* ws, float* total_norm, u3d_stream_t stream);

/* =====================================================================================
 * R16  detection evaluation of a whole validation pass (csrc/evalmap.hip): mAP / mAR at IoU thresholds as the reference's
 *      indoor_eval computes them (unidet3d/indoor_eval.py:56-161 eval_det_cls, :8-53 average_precision; the host restatement is
 *      unidet3d_amd/evaluation.py).  One dataset's pass is packed image after image: det_boxes [D][7], det_scores [D], det_labels
 *      int32 [D], det_off int32 [I+1]; gt_boxes [G][7], gt_labels int32 [G], gt_off int32 [I+1] (offsets ascending from 0).  Boxes
 *      are bottom-centre depth boxes (x, y, z_bottom, dx, dy, dz, yaw), six-column boxes packed with yaw 0.  C classes
 *      (<= U3D_EVAL_MAX_CLASSES), T thresholds (<= U3D_EVAL_MAX_THR); a label outside [0, C) matches nothing, is not counted and
 *      sorts behind every class.  Zero sizes are valid; nothing is launched for an empty dimension.  Integer atomics only; every
 *      floating-point sum has a fixed order: results are bit-reproducible.  Added entry points: U3D_ABI_VERSION is unchanged.
 * ===================================================================================== */
#define U3D_EVAL_MAX_CLASSES 1024
#define U3D_EVAL_MAX_THR 8
#define U3D_EVAL_GT_CHUNK 128    /* ground truths of an image staged in LDS at a time (an image may have more) */
int u3d_eval_gt_chunk(void);     /* U3D_EVAL_GT_CHUNK of the library that was loaded */
/* iou_max [D]: the largest 3-D IoU (BEV intersection x height overlap over the union of the volumes, union clamped at 1e-8) of the
 * detection with a ground truth of its class in its image, -inf when there is none; jmax int32 [D]: the packed index of that
 * ground truth -- the first maximum of a strict '>' scan in ground-truth order (indoor_eval.py:132-139) -- or -1.  A pair whose
 * two headings are both exactly 0 takes the axis-aligned fp32 expression in evaluation.boxes_iou_3d's operation order (bit-equal
 * to it); any other pair the rotated-rectangle intersection, evaluated in fp64 and rounded once.  n_gt / n_det int32 [C]: the
 * class histograms (zeroed here).  ws is not used (u3d_eval_match_ws_bytes returns 0; NULL is fine). */
int u3d_eval_match(const float* det_boxes, const int32_t* det_labels, const int32_t* det_off, const float* gt_boxes, const int32_t* gt_labels,
                   const int32_t* gt_off, int64_t D, int64_t G, int64_t I, int C, float* iou_max, int32_t* jmax, int32_t* n_gt, int32_t* n_det,
                   void* ws, u3d_stream_t stream);
int64_t u3d_eval_match_ws_bytes(int64_t D, int64_t G);
/* perm int32 [D]: the detections in evaluation order -- class ascending, score descending, ties by packed index (stable): one
 * u3d_sort_u64 over class << 32 | order-preserving uint of -score.  Any finite score orders correctly, -0 ties with +0, NaN scores
 * come last in their class (where numpy's sort puts them). */
int u3d_eval_order(const float* det_scores, const int32_t* det_labels, int64_t D, int C, int32_t* perm, void* ws, u3d_stream_t stream);
int64_t u3d_eval_order_ws_bytes(int64_t D);
/* Every (class, threshold) pair from the outputs of the two calls above.  The detection at sorted rank r is a true positive at
 * threshold t iff iou_max > thr[t] and r is the smallest rank among the detections with iou_max > thr[t] that name the same jmax
 * (integer atomicMin per (ground truth, threshold)); everything else is a false positive.  Cumulative counts, recall = tp / n_gt and
 * precision = tp / max(tp + fp, eps) in fp64 over the class segment; AP = the all-points area of average_precision(mode='area').
 * thr_host: T floats on the HOST (passed on as a kernel argument).  ap / rec float [T][C] (rec: the last recall of the segment): NaN
 * for a class with detections and no ground truth (the host's 0 / 0), 0 for a class without detections.  tp_flag uint8 [T][D] and
 * tp_cum int32 [T][D] (both nullable): flag and cumulative true positives inside the class segment, by sorted rank (the false
 * positives up to rank r of a segment that starts at s are r - s + 1 - tp_cum); ranks of labels outside [0, C) are not written. */
int u3d_eval_sweep(const float* iou_max, const int32_t* jmax, const int32_t* perm, const int32_t* n_gt, const int32_t* n_det,
                   const float* thr_host, int64_t D, int64_t G, int C, int T, float* ap, float* rec, uint8_t* tp_flag, int32_t* tp_cum,
                   void* ws, u3d_stream_t stream);
int64_t u3d_eval_sweep_ws_bytes(int64_t D, int64_t G, int T);

#ifdef __cplusplus
}
#endif
#endif /* U3D_H_ */
