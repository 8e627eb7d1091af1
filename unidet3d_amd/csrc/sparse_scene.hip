// Per-scene operations on sparse tensors (include/u3d.h section S3): where each scene's rows start in the canonical row order, the
// top-k rows of every scene by a score (the `_prune` step of generative necks), and global max / average pooling per scene (spconv's
// SparseGlobalMaxPool / SparseGlobalAvgPool).  Everything runs a whole batch in one chain of launches without a host read.
//  * scene ranges: thread = row, compares its batch index with its predecessor's and writes every entry in between: each entry of
//    offsets is written exactly once, no atomics on it, no memset of it;
//  * top-k: a radix select on the order-preserving integer image of the scores -- four 8-bit histogram passes (LDS counters, one integer
//    atomic per non-empty bin and workgroup, several workgroups per scene) give each scene's threshold key T and the rows strictly above
//    it; one stable pass keeps key > T plus the first k - above rows with key == T, positions from block counts, a scan and the wave-64
//    ballot prefix of rb_compact.h.  Integer only: one result whatever the arrival order;
//  * pooling: partials per chunk of a fixed row count (16-byte loads, a group of lanes per row, LDS only for the cross-group combine),
//    then one workgroup per scene over its chunks in ascending order, in consecutive runs that meet in the same fixed tree.  The average
//    accumulates in fp64.  The backward is a gather: every element of dx written once.
// Scene ranges are clamped to [0, n] wherever they are read: a tensor that is not in canonical order (flagged by scene_offsets_k) gives
// wrong values, never an access outside a tensor.
#include "rb_compact.h"

// dy * (1 / n_b) rounds on its own, as in sparse_pool.hip
#pragma clang fp contract(off)

namespace u3d {

constexpr int TK_ROWS = RB_T;           // rows of one workgroup in one trip of a histogram pass, and of a block of the stable pass
constexpr int TK_BLOCKS = 512;          // workgroups of one histogram pass over all scenes (two per CU)
constexpr int PL_CHUNKS = 1024;         // chunks the pooling plan aims at over all scenes (four workgroups per CU)

// ---- scene ranges -------------------------------------------------------------------------------------------------------------------
// thread i < n: row i; thread n: the end (batch index B).  Writes offsets[j] = i for every j in (batch of row i - 1, batch of row i].
__global__ __launch_bounds__(RB_T) void scene_offsets_k(const int32_t* __restrict__ coords, int64_t n, int B, int32_t* __restrict__ offsets,
                                                        int32_t* flag) {
    const int64_t i = (int64_t)blockIdx.x * RB_T + threadIdx.x;
    if (i > n) return;
    const int b = i < n ? coords[i * 4] : B;
    const int p = i > 0 ? coords[(i - 1) * 4] : -1;
    int bad = 0;
    if (i < n && (unsigned)b >= (unsigned)B) bad |= 2;
    if (i < n && i > 0 && b < p) bad |= 1;
    if (bad) atomicOr(flag, bad);
    const int hi = i < n ? min(max(b, 0), B - 1) : B;         // (clamped: a wrong batch index never forms an address outside offsets)
    const int lo = i > 0 ? min(max(p, 0), B - 1) : -1;
    for (int j = lo + 1; j <= hi; ++j) offsets[j] = (int32_t)i;
}

// the rows [lo, hi) of scene b, inside [0, n] whatever offsets holds
__device__ __forceinline__ void scene_range(const int32_t* __restrict__ offsets, int64_t n, int b, int64_t& lo, int64_t& hi) {
    lo = min(max((int64_t)offsets[b], (int64_t)0), n);
    hi = min(max((int64_t)offsets[b + 1], lo), n);
}

// ---- top-k: keys ---------------------------------------------------------------------------------------------------------------------
// the order-preserving integer image of a score's bits: every NaN is the one largest key, -0.0 is +0.0, denormals keep their value (no
// floating-point instruction touches a score); largest == 0 reverses the order of the numbers and leaves the NaNs on top
__device__ __forceinline__ uint32_t topk_key(uint32_t u, int largest) {
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
    if (u == 0x80000000u) u = 0u;
    const uint32_t k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return largest ? k : ~k;
}

// One step of the select, by all RB_T threads of a workgroup: hist = the 256 counters of the rows that match `prefix` so far, by their
// next digit.  Finds the digit d with (rows of a larger digit) < remain <= (rows of digit >= d), appends it to prefix (at `shift`),
// takes the rows of a larger digit off remain; eq = the rows of digit d.  remain == 0 (nothing to keep) picks 255 and changes nothing:
// the threshold then ends as the NaN key with no tie wanted.
__device__ __forceinline__ void select_step(const int32_t* __restrict__ hist, int shift, uint32_t& prefix, int& remain, int& eq, int* s_w,
                                            int* s_pick) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int d = 255 - (int)threadIdx.x;
    const int v = hist[d];
    int incl = v;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const int t = __shfl_up(incl, s, 64);
        if (lane >= s) incl += t;
    }
    if (lane == 63) s_w[wave] = incl;
    if (threadIdx.x == 0) { s_pick[0] = 255; s_pick[1] = 0; s_pick[2] = v; }
    __syncthreads();
    int ge = incl;
#pragma unroll
    for (int w = 0; w < RB_T / 64; ++w) if (w < wave) ge += s_w[w];
    const int gt = ge - v;
    if (gt < remain && remain <= ge) { s_pick[0] = d; s_pick[1] = gt; s_pick[2] = v; }
    __syncthreads();
    prefix |= (uint32_t)s_pick[0] << shift;
    remain -= s_pick[1];
    eq = s_pick[2];
    __syncthreads();
}

// the state of scene b after pass `pass` - 1 (prefix, remain): from k for the first, from st for a later one; st: [3][B][2]
__device__ __forceinline__ void select_state(const int32_t* __restrict__ st, const int32_t* __restrict__ k, int B, int b, int64_t nb, int pass,
                                             uint32_t& prefix, int& remain) {
    if (pass <= 0) {
        prefix = 0u;
        remain = (int)min((int64_t)max(k[b], 0), nb);
    } else {
        prefix = (uint32_t)st[((pass - 1) * B + b) * 2];
        remain = st[((pass - 1) * B + b) * 2 + 1];
    }
}

// Histogram pass PASS of scene blockIdx.y: digit (24 - 8 PASS) of the keys whose higher digits equal the prefix.  The prefix itself comes
// from the previous pass's counters: every workgroup takes that step for itself (256 loads), workgroup 0 of the scene records it.
template <int PASS>
__global__ __launch_bounds__(RB_T) void topk_hist_k(const uint32_t* __restrict__ scores, const int32_t* __restrict__ offsets,
                                                    const int32_t* __restrict__ k, int64_t n, int B, int largest, int32_t* hist, int32_t* st) {
    __shared__ int s_hist[256];
    __shared__ int s_w[RB_T / 64];
    __shared__ int s_pick[3];
    const int b = blockIdx.y;
    int64_t lo, hi;
    scene_range(offsets, n, b, lo, hi);
    uint32_t prefix = 0u;
    if (PASS > 0) {
        int remain, eq;
        select_state(st, k, B, b, hi - lo, PASS - 1, prefix, remain);
        select_step(hist + ((int64_t)(PASS - 1) * B + b) * 256, 32 - 8 * PASS, prefix, remain, eq, s_w, s_pick);
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            st[((PASS - 1) * B + b) * 2] = (int32_t)prefix;
            st[((PASS - 1) * B + b) * 2 + 1] = remain;
        }
    }
    s_hist[threadIdx.x] = 0;
    __syncthreads();
    for (int64_t base = lo + (int64_t)blockIdx.x * TK_ROWS; base < hi; base += (int64_t)gridDim.x * TK_ROWS) {
        const int64_t r = base + threadIdx.x;
        if (r < hi) {
            const uint32_t key = topk_key(scores[r], largest);
            const bool match = PASS == 0 || ((key ^ prefix) >> (PASS == 0 ? 0 : 32 - 8 * PASS)) == 0u;
            if (match) atomicAdd(&s_hist[(key >> (24 - 8 * PASS)) & 255u], 1);
        }
    }
    __syncthreads();
    const int v = s_hist[threadIdx.x];
    if (v) atomicAdd(&hist[((int64_t)PASS * B + b) * 256 + threadIdx.x], v);
}

// what the stable pass reads of scene b: sel[b] = (T, ties wanted, ties of the scenes before, kept ties of the scenes before)
constexpr int SEL = 4;

// one workgroup: the last select step of every scene, the prefix sums over the scenes, the kept count and the order flag
__global__ __launch_bounds__(RB_T) void topk_final_k(const int32_t* __restrict__ offsets, const int32_t* __restrict__ k, int64_t n, int B,
                                                     const int32_t* __restrict__ hist, const int32_t* __restrict__ st,
                                                     const int32_t* __restrict__ flag, int32_t* __restrict__ sel, int32_t* __restrict__ result) {
    __shared__ int s_w[RB_T / 64];
    __shared__ int s_pick[3];
    int ties_before = 0, kept_ties_before = 0;
    int64_t total = 0;
    for (int b = 0; b < B; ++b) {
        int64_t lo, hi;
        scene_range(offsets, n, b, lo, hi);
        uint32_t prefix;
        int remain, eq;
        select_state(st, k, B, b, hi - lo, 3, prefix, remain);
        total += min((int64_t)max(k[b], 0), hi - lo);
        select_step(hist + ((int64_t)3 * B + b) * 256, 0, prefix, remain, eq, s_w, s_pick);
        if (threadIdx.x == 0) {
            sel[b * SEL] = (int32_t)prefix;
            sel[b * SEL + 1] = remain;
            sel[b * SEL + 2] = ties_before;
            sel[b * SEL + 3] = kept_ties_before;
        }
        ties_before += eq;
        kept_ties_before += remain;
    }
    if (threadIdx.x == 0) {
        result[0] = (int32_t)min(total, n);
        result[1] = flag[0];
    }
}

// the scene of a row by its batch index, inside [0, B)
__device__ __forceinline__ int row_scene(const int32_t* __restrict__ coords, int64_t r, int B) { return min(max(coords[r * 4], 0), B - 1); }

// block counts of the stable pass: list 0 the rows above their scene's threshold, list 1 the rows on it
__global__ __launch_bounds__(RB_T) void topk_count_k(const uint32_t* __restrict__ scores, const int32_t* __restrict__ coords, int64_t n, int B,
                                                     int largest, const int32_t* __restrict__ sel, int nblk, int32_t* __restrict__ block_cnt) {
    const int64_t r = (int64_t)blockIdx.x * RB_T + threadIdx.x;
    bool above = false, tie = false;
    if (r < n) {
        const uint32_t key = topk_key(scores[r], largest), T = (uint32_t)sel[row_scene(coords, r, B) * SEL];
        above = key > T;
        tie = key == T;
    }
    const int ca = __syncthreads_count(above), ct = __syncthreads_count(tie);
    if (threadIdx.x == 0) { block_cnt[blockIdx.x] = ca; block_cnt[nblk + blockIdx.x] = ct; }
}

// mask, pos and kept of every row: a row above the threshold is kept, a row on it while its rank among its scene's ties is below the
// ties wanted; position = the rows above before it + the kept ties before it (those of earlier scenes + min(its tie rank, ties wanted))
__global__ __launch_bounds__(RB_T) void topk_write_k(const uint32_t* __restrict__ scores, const int32_t* __restrict__ coords, int64_t n, int B,
                                                     int largest, const int32_t* __restrict__ sel, int nblk, const int32_t* __restrict__ block_base,
                                                     uint8_t* __restrict__ mask, int32_t* __restrict__ kept, int32_t* __restrict__ pos) {
    __shared__ int s_a[RB_T / 64];
    __shared__ int s_t[RB_T / 64];
    const int64_t r = (int64_t)blockIdx.x * RB_T + threadIdx.x;
    bool above = false, tie = false;
    int want = 0, ties_before = 0, kept_ties_before = 0;
    if (r < n) {
        const int32_t* s = sel + row_scene(coords, r, B) * SEL;
        const uint32_t key = topk_key(scores[r], largest), T = (uint32_t)s[0];
        above = key > T;
        tie = key == T;
        want = s[1]; ties_before = s[2]; kept_ties_before = s[3];
    }
    const int ra = block_base[blockIdx.x] + rb_block_rank(above, s_a);
    const int rt = block_base[nblk + blockIdx.x] + rb_block_rank(tie, s_t) - ties_before;      // rank among the scene's ties
    if (r >= n) return;
    const bool keep = above || (tie && rt < want);
    const int at = ra + kept_ties_before + min(max(rt, 0), want);
    mask[r] = keep ? 1 : 0;
    pos[r] = keep ? at : -1;
    if (keep && (uint64_t)(int64_t)at < (uint64_t)n) kept[at] = (int32_t)r;      // (at < n in canonical order; the test guards a wrong order)
}

// ---- global pooling -------------------------------------------------------------------------------------------------------------------
// a chunk = R consecutive rows of one scene (the last of a scene may hold fewer); chunks are numbered scene by scene
__device__ __forceinline__ int64_t scene_chunks(int64_t lo, int64_t hi, int R) { return (hi - lo + R - 1) / R; }

// the element that the maximum keeps of two: a NaN before a number, the larger number, on a tie (and among NaNs) the lower row --
// what sparse_pool.hip's take_max leaves after walking the rows in ascending order
__device__ __forceinline__ void max_merge(float& hv, int& hr, float v, int r) {
    const bool vn = v != v, hn = hv != hv;
    const bool rep = hr < 0 || (vn != hn ? vn : (!vn && v != hv ? v > hv : r < hr));
    hv = rep ? v : hv;
    hr = rep ? r : hr;
}

struct Max4 { float4 v; int4 r; };
struct Sum4 { double x, y, z, w; };

__device__ __forceinline__ void merge(Max4& h, const Max4& o) {
    if (o.r.x >= 0) max_merge(h.v.x, h.r.x, o.v.x, o.r.x);
    if (o.r.y >= 0) max_merge(h.v.y, h.r.y, o.v.y, o.r.y);
    if (o.r.z >= 0) max_merge(h.v.z, h.r.z, o.v.z, o.r.z);
    if (o.r.w >= 0) max_merge(h.v.w, h.r.w, o.v.w, o.r.w);
}
__device__ __forceinline__ void merge(Sum4& h, const Sum4& o) { h.x += o.x; h.y += o.y; h.z += o.z; h.w += o.w; }
// a row BEHIND every row the accumulator has seen (a group walks its rows in ascending order): take_max itself, no row compare
__device__ __forceinline__ void max_next(float& hv, int& hr, float v, int r) {
    const bool rep = hr < 0 || v > hv || (v != v && hv == hv);
    hv = rep ? v : hv;
    hr = rep ? r : hr;
}
__device__ __forceinline__ void take(Max4& h, const float4& v, int r) {
    max_next(h.v.x, h.r.x, v.x, r); max_next(h.v.y, h.r.y, v.y, r); max_next(h.v.z, h.r.z, v.z, r); max_next(h.v.w, h.r.w, v.w, r);
}
__device__ __forceinline__ void take(Sum4& h, const float4& v, int) { h.x += (double)v.x; h.y += (double)v.y; h.z += (double)v.z; h.w += (double)v.w; }
__device__ __forceinline__ void clear(Max4& h) { h.v = make_float4(0.f, 0.f, 0.f, 0.f); h.r = make_int4(-1, -1, -1, -1); }
__device__ __forceinline__ void clear(Sum4& h) { h.x = h.y = h.z = h.w = 0.0; }

constexpr int PL_ROWS = 8;      // row loads of one group in flight

// first pass: workgroup = chunk.  lg = log2(lanes per row); group g of the 256 >> lg groups walks the rows g, g + G, ... of the chunk in
// ascending order, lane l of it the columns 4 l (+ 256 per trip of the column loop); the groups' results meet in LDS, a fixed tree.
template <class ACC>
__global__ __launch_bounds__(RB_T) void scene_pool_part_k(const float4* __restrict__ x, const int32_t* __restrict__ offsets, int64_t n, int B,
                                                          int C4, int lg, int R, ACC* __restrict__ part) {
    __shared__ ACC s_acc[RB_T];
    // the chunk's scene and rows
    int64_t r0 = 0, r1 = 0;
    {
        int64_t q = blockIdx.x;
        bool found = false;
        for (int b = 0; b < B && !found; ++b) {
            int64_t lo, hi;
            scene_range(offsets, n, b, lo, hi);
            const int64_t c = scene_chunks(lo, hi, R);
            if (q < c) { r0 = lo + q * R; r1 = min(r0 + R, hi); found = true; }
            q -= c;
        }
        if (!found) return;          // (uniform over the workgroup: past the last chunk)
    }
    const int L = 1 << lg, G = RB_T >> lg;
    const int g = threadIdx.x >> lg, l = threadIdx.x & (L - 1);
    for (int cb = 0; cb < C4; cb += L) {
        const int c = cb + l;
        ACC acc;
        clear(acc);
        if (c < C4) {
            for (int64_t r = r0 + g; r < r1; r += (int64_t)G * PL_ROWS) {
                float4 v[PL_ROWS];
#pragma unroll
                for (int u = 0; u < PL_ROWS; ++u)
                    if (r + (int64_t)u * G < r1) v[u] = x[(r + (int64_t)u * G) * C4 + c];
#pragma unroll
                for (int u = 0; u < PL_ROWS; ++u)
                    if (r + (int64_t)u * G < r1) take(acc, v[u], (int)(r + (int64_t)u * G));
            }
        }
        s_acc[threadIdx.x] = acc;
        __syncthreads();
        for (int s = G >> 1; s >= 1; s >>= 1) {
            if (g < s) {
                merge(acc, s_acc[threadIdx.x + (s << lg)]);
                s_acc[threadIdx.x] = acc;
            }
            __syncthreads();
        }
        if (g == 0 && c < C4) part[(int64_t)blockIdx.x * C4 + c] = acc;
    }
}

// what a scene's accumulator becomes: the maximum and its row (+0.0 and -1 for an empty scene), or sum / n_b rounded once (+0.0)
__device__ __forceinline__ void finish(const Max4& a, int64_t, float4* y, int4* arg, int64_t at) { y[at] = a.v; arg[at] = a.r; }
__device__ __forceinline__ void finish(const Sum4& a, int64_t nb, float4* y, int4*, int64_t at) {
    const double d = (double)nb;
    y[at] = nb > 0 ? make_float4((float)(a.x / d), (float)(a.y / d), (float)(a.z / d), (float)(a.w / d)) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// second pass: workgroup = scene, lanes as in the first pass.  The scene's chunks in ascending order, cut into G consecutive runs: group g
// adds up (merges) run g chunk by chunk, the runs meet in LDS in the same fixed tree.  A chain of ceil(chunks / G) dependent steps, not of
// `chunks`: one workgroup per scene stays short when B = 1.
template <class ACC>
__global__ __launch_bounds__(RB_T) void scene_pool_fin_k(const ACC* __restrict__ part, const int32_t* __restrict__ offsets, int64_t n, int B, int C4,
                                                         int lg, int R, int64_t Q, float4* __restrict__ y, int4* __restrict__ arg) {
    __shared__ ACC s_acc[RB_T];
    const int b = blockIdx.x;
    int64_t q0 = 0, lo, hi;
    for (int j = 0; j < b; ++j) {
        scene_range(offsets, n, j, lo, hi);
        q0 += scene_chunks(lo, hi, R);
    }
    scene_range(offsets, n, b, lo, hi);
    const int64_t q1 = min(q0 + scene_chunks(lo, hi, R), Q);          // (Q: the chunks that exist, whatever offsets holds)
    const int L = 1 << lg, G = RB_T >> lg;
    const int g = threadIdx.x >> lg, l = threadIdx.x & (L - 1);
    const int64_t run = q1 > q0 ? (q1 - q0 + G - 1) / G : 0;
    const int64_t qa = min(q0 + g * run, q1), qb = min(qa + run, q1);
    for (int cb = 0; cb < C4; cb += L) {
        const int c = cb + l;
        ACC acc;
        clear(acc);
        if (c < C4) {
            for (int64_t q = qa; q < qb; q += PL_ROWS) {
                ACC v[PL_ROWS];
#pragma unroll
                for (int u = 0; u < PL_ROWS; ++u)
                    if (q + u < qb) v[u] = part[(q + u) * C4 + c];
#pragma unroll
                for (int u = 0; u < PL_ROWS; ++u)
                    if (q + u < qb) merge(acc, v[u]);
            }
        }
        s_acc[threadIdx.x] = acc;
        __syncthreads();
        for (int s = G >> 1; s >= 1; s >>= 1) {
            if (g < s) {
                merge(acc, s_acc[threadIdx.x + (s << lg)]);
                s_acc[threadIdx.x] = acc;
            }
            __syncthreads();
        }
        if (g == 0 && c < C4) finish(acc, hi - lo, y, arg, (int64_t)b * C4 + c);
    }
}

// backward, gather form: thread t serves row t >> lg, columns 4 (t & (lanes - 1)) + 256 i; every element of dx written once
template <int MODE>
__global__ __launch_bounds__(RB_T) void scene_pool_bwd_k(const float4* __restrict__ dy, const int32_t* __restrict__ coords,
                                                         const int32_t* __restrict__ offsets, const int4* __restrict__ arg, int64_t n, int B, int C4,
                                                         int lg, float4* __restrict__ dx) {
    const int64_t t = (int64_t)blockIdx.x * RB_T + threadIdx.x;
    const int64_t i = t >> lg;
    if (i >= n) return;
    const int b = coords[i * 4];
    const bool in = (unsigned)b < (unsigned)B;
    float inv = 0.f;
    if (MODE == U3D_POOL_AVG && in) {
        int64_t lo, hi;
        scene_range(offsets, n, b, lo, hi);
        inv = 1.0f / (float)(hi > lo ? hi - lo : 1);
    }
    for (int c = (int)(t & ((1 << lg) - 1)); c < C4; c += 1 << lg) {
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (in) {
            const float4 g = dy[(int64_t)b * C4 + c];
            if (MODE == U3D_POOL_MAX) {
                const int4 a = arg[(int64_t)b * C4 + c];
                o = make_float4(a.x == i ? g.x : 0.f, a.y == i ? g.y : 0.f, a.z == i ? g.z : 0.f, a.w == i ? g.w : 0.f);
            } else {
                o = make_float4(g.x * inv, g.y * inv, g.z * inv, g.w * inv);
            }
        }
        dx[i * C4 + c] = o;
    }
}

// lanes per row: the power of two that covers C / 4, one wave at most (sparse_pool.hip's rule)
static int lanes_log2(int C) {
    int lg = 0;
    while (lg < 6 && (4 << lg) < C) ++lg;
    return lg;
}

static int topk_blocks(int64_t n, int B) {
    const int64_t cap = TK_BLOCKS / B > 1 ? TK_BLOCKS / B : 1;
    const int64_t need = ceil_div(n, TK_ROWS);
    return (int)(need < 1 ? 1 : (need < cap ? need : cap));
}

static int pool_chunk_rows(int64_t n) {
    const int64_t r = ceil_div(ceil_div(n, PL_CHUNKS), 64) * 64;
    return (int)(r < 64 ? 64 : r);
}

// the contract every entry point of this file shares, checked before any HIP call
static int check_scene(const char* what, bool null, int64_t n, int B) {
    if (null || n <= 0 || B <= 0) {
        set_error("%s: NULL pointer, no rows (n = %lld) or no scenes (B = %d)", what, (long long)n, B);
        return U3D_EINVAL;
    }
    if (n >= 0x80000000LL) { set_error("%s: %lld rows exceed 32-bit row numbers", what, (long long)n); return U3D_EUNSUPPORTED; }
    if (B > 65535) { set_error("%s: %d scenes exceed a launch of 65535 scene workgroups", what, B); return U3D_EUNSUPPORTED; }
    return U3D_OK;
}

static int check_pool_shape(const char* what, int C, int mode) {
    if (mode != U3D_POOL_MAX && mode != U3D_POOL_AVG) { set_error("%s: mode %d is neither U3D_POOL_MAX nor U3D_POOL_AVG", what, mode); return U3D_EINVAL; }
    if (C < 4 || C > 512 || C % 4) { set_error("%s: width %d unsupported (a multiple of 4 in 4..512)", what, C); return U3D_EUNSUPPORTED; }
    return U3D_OK;
}

// workspace of u3d_scene_topk, in int32: [4][B][256] counters | [3][B][2] states | [B][SEL] | [2][nblk] counts | [2][nblk] bases | totals
struct TopkWs { int64_t hist, st, sel, bc, bb, tot, end; };
static TopkWs topk_ws(int64_t n, int B) {
    const int64_t nblk = ceil_div(n, RB_T);
    TopkWs w;
    w.hist = 0;
    w.st = w.hist + (int64_t)4 * B * 256;
    w.sel = w.st + (int64_t)3 * B * 2;
    w.bc = w.sel + (int64_t)B * SEL;
    w.bb = w.bc + 2 * nblk;
    w.tot = w.bb + 2 * nblk;
    w.end = w.tot + 64;
    return w;
}

}  // namespace u3d

using namespace u3d;

extern "C" {

int u3d_scene_offsets(const int32_t* coords, int64_t n, int B, int32_t* offsets, int32_t* flag, u3d_stream_t stream) {
    const int rc = check_scene("scene_offsets", !coords || !offsets || !flag, n, B);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(U3D_K_RULEBOOK, s, 0.0);
    if (hipMemsetAsync(flag, 0, sizeof(int32_t), s) != hipSuccess) return check_launch("scene_offsets (flag)");
    hipLaunchKernelGGL(scene_offsets_k, dim3((unsigned)ceil_div(n + 1, RB_T)), dim3(RB_T), 0, s, coords, n, B, offsets, flag);
    return check_launch("scene_offsets");
}

int u3d_scene_topk_plan(int64_t n, int B, int* rows_per_block, int* blocks_per_scene) {
    const int rc = check_scene("scene_topk_plan", false, n, B);
    if (rc) return rc;
    if (rows_per_block) *rows_per_block = TK_ROWS;
    if (blocks_per_scene) *blocks_per_scene = topk_blocks(n, B);
    return U3D_OK;
}

int64_t u3d_scene_topk_ws_bytes(int64_t n, int B) {
    if (n <= 0 || B <= 0) return 0;
    return topk_ws(n, B).end * 4;
}

int u3d_scene_topk(const float* scores, const int32_t* coords, const int32_t* offsets, const int32_t* flag, const int32_t* k, int64_t n, int B,
                   int largest, uint8_t* mask, int32_t* kept, int32_t* pos, int32_t* result, void* ws, u3d_stream_t stream) {
    const int rc = check_scene("scene_topk", !scores || !coords || !offsets || !flag || !k || !mask || !kept || !pos || !result || !ws, n, B);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(U3D_K_RULEBOOK, s, 0.0);
    const TopkWs w = topk_ws(n, B);
    int32_t* base = (int32_t*)ws;
    int32_t *hist = base + w.hist, *st = base + w.st, *sel = base + w.sel, *bc = base + w.bc, *bb = base + w.bb, *tot = base + w.tot;
    const uint32_t* sc = reinterpret_cast<const uint32_t*>(scores);
    const int lg = largest ? 1 : 0;
    if (hipMemsetAsync(hist, 0, (size_t)(w.st - w.hist) * 4, s) != hipSuccess) return check_launch("scene_topk (counters)");
    const dim3 grid((unsigned)topk_blocks(n, B), (unsigned)B);
    hipLaunchKernelGGL((topk_hist_k<0>), grid, dim3(RB_T), 0, s, sc, offsets, k, n, B, lg, hist, st);
    hipLaunchKernelGGL((topk_hist_k<1>), grid, dim3(RB_T), 0, s, sc, offsets, k, n, B, lg, hist, st);
    hipLaunchKernelGGL((topk_hist_k<2>), grid, dim3(RB_T), 0, s, sc, offsets, k, n, B, lg, hist, st);
    hipLaunchKernelGGL((topk_hist_k<3>), grid, dim3(RB_T), 0, s, sc, offsets, k, n, B, lg, hist, st);
    hipLaunchKernelGGL(topk_final_k, dim3(1), dim3(RB_T), 0, s, offsets, k, n, B, (const int32_t*)hist, (const int32_t*)st, flag, sel, result);
    const int nblk = (int)ceil_div(n, RB_T);
    hipLaunchKernelGGL(topk_count_k, dim3(nblk), dim3(RB_T), 0, s, sc, coords, n, B, lg, (const int32_t*)sel, nblk, bc);
    hipLaunchKernelGGL(rb_scan_k, dim3(2), dim3(RB_T), 0, s, (const int32_t*)bc, nblk, bb, tot);
    hipLaunchKernelGGL(topk_write_k, dim3(nblk), dim3(RB_T), 0, s, sc, coords, n, B, lg, (const int32_t*)sel, nblk, (const int32_t*)bb, mask, kept, pos);
    return check_launch("scene_topk");
}

int u3d_scene_pool_plan(int64_t n, int B, int C, int* rows_per_chunk, int64_t* max_chunks) {
    int rc = check_scene("scene_pool_plan", false, n, B);
    if (!rc) rc = check_pool_shape("scene_pool_plan", C, U3D_POOL_MAX);
    if (rc) return rc;
    const int R = pool_chunk_rows(n);
    if (rows_per_chunk) *rows_per_chunk = R;
    if (max_chunks) *max_chunks = ceil_div(n, R) + B;          // every scene may end in a partial chunk
    return U3D_OK;
}

int64_t u3d_scene_pool_ws_bytes(int64_t n, int B, int C) {
    if (n <= 0 || B <= 0 || C <= 0) return 0;
    return (ceil_div(n, pool_chunk_rows(n)) + B) * (int64_t)C * 8;      // per chunk and column: a double, or a float and a row
}

int u3d_scene_pool_fwd(const float* x, const int32_t* offsets, int64_t n, int B, int C, int mode, float* y, int32_t* arg, void* ws,
                       u3d_stream_t stream) {
    int rc = check_scene("scene_pool_fwd", !x || !offsets || !y || !ws || (mode == U3D_POOL_MAX && !arg), n, B);
    if (!rc) rc = check_pool_shape("scene_pool_fwd", C, mode);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(U3D_K_POOL, s, 0.0);
    const int lg = lanes_log2(C), R = pool_chunk_rows(n), C4 = C / 4;
    const int64_t Q = ceil_div(n, R) + B;
    const float4* x4 = reinterpret_cast<const float4*>(x);
    if (mode == U3D_POOL_MAX) {
        hipLaunchKernelGGL((scene_pool_part_k<Max4>), dim3((unsigned)Q), dim3(RB_T), 0, s, x4, offsets, n, B, C4, lg, R, (Max4*)ws);
        hipLaunchKernelGGL((scene_pool_fin_k<Max4>), dim3((unsigned)B), dim3(RB_T), 0, s, (const Max4*)ws, offsets, n, B, C4, lg, R, Q,
                           reinterpret_cast<float4*>(y), reinterpret_cast<int4*>(arg));
    } else {
        hipLaunchKernelGGL((scene_pool_part_k<Sum4>), dim3((unsigned)Q), dim3(RB_T), 0, s, x4, offsets, n, B, C4, lg, R, (Sum4*)ws);
        hipLaunchKernelGGL((scene_pool_fin_k<Sum4>), dim3((unsigned)B), dim3(RB_T), 0, s, (const Sum4*)ws, offsets, n, B, C4, lg, R, Q,
                           reinterpret_cast<float4*>(y), reinterpret_cast<int4*>(arg));
    }
    return check_launch("scene_pool_fwd");
}

int u3d_scene_pool_bwd(const float* dy, const int32_t* coords, const int32_t* offsets, const int32_t* arg, int64_t n, int B, int C, int mode,
                       float* dx, u3d_stream_t stream) {
    int rc = check_scene("scene_pool_bwd", !dy || !coords || !offsets || !dx || (mode == U3D_POOL_MAX && !arg), n, B);
    if (!rc) rc = check_pool_shape("scene_pool_bwd", C, mode);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(U3D_K_POOL, s, 0.0);
    const int lg = lanes_log2(C), C4 = C / 4;
    const dim3 grid((unsigned)ceil_div(n << lg, RB_T));
    const float4* g4 = reinterpret_cast<const float4*>(dy);
    if (mode == U3D_POOL_MAX)
        hipLaunchKernelGGL((scene_pool_bwd_k<U3D_POOL_MAX>), grid, dim3(RB_T), 0, s, g4, coords, offsets, reinterpret_cast<const int4*>(arg), n, B, C4, lg,
                           reinterpret_cast<float4*>(dx));
    else
        hipLaunchKernelGGL((scene_pool_bwd_k<U3D_POOL_AVG>), grid, dim3(RB_T), 0, s, g4, coords, offsets, reinterpret_cast<const int4*>(arg), n, B, C4, lg,
                           reinterpret_cast<float4*>(dx));
    return check_launch("scene_pool_bwd");
}

}  // extern "C"
