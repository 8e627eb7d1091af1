// K-post: inference post-processing of one scene on the device:
//   * class-wise greedy NMS of axis-aligned boxes -- unidet3d/unidet3d.py:595-650: fast_nms=True is
//     mmcv.ops.nms3d_normal (mmcv @780ffed, ops/csrc/common/cuda/iou3d_cuda_kernel.cuh `iou_normal`: IoU of the
//     (x, y, dx, dy) rectangles, z and heading ignored), fast_nms=False is mmdet3d 1.4.0 aligned_3d_nms (3-D IoU of
//     the corner boxes); both visit a class in descending score order;
//   * superpoint trimming of the surviving boxes -- unidet3d/unidet3d.py:540-593 + get_face_distances :652-677:
//     point-in-box test, per-superpoint inside ratio, delete (< low) / add (> up) whole superpoints, min/max of
//     the selected points.
// Both are integer / comparison work on small inputs: bit-exact against oracle/postproc.py, which repeats the same
// fp32 operation order (this file is built with -ffp-contract=off so no multiply-add is fused).
#include <math.h>

#include "u3d_common.h"

namespace u3d {

constexpr int NMS_MAX = 4400;          // 9 LDS words per box: 158 KB of the CU's 160 KB (launches above 64 KB opt in, see lds_opt_in)
constexpr int NMS_ROT_MAX = 3600;      // 11 LDS words per box

// MODE 0: BEV IoU of (cx, cy, cz, dx, dy, dz) boxes, suppress when iou > thr           (mmcv nms3d_normal / iou_normal)
// MODE 1: 3-D IoU of (x1, y1, z1, x2, y2, z2) boxes, survive only when iou <= thr       (mmdet3d aligned_3d_nms: a 0/0 IoU
//         of two zero-volume boxes is NaN there and NaN <= thr is false, so such a box is dropped)
// The IoU arithmetic lives in the two functions below; nms_k (one scene) and nms_seg_k (batched, one class segment per
// workgroup) both call them, so their keep flags agree by construction.
struct NmsTerms { float x1, x2, y1, y2, z1, z2, ar; };

template <int MODE>
__device__ __forceinline__ NmsTerms nms_terms(const float* b) {
    NmsTerms t;
    if (MODE == 0) {
        t.x1 = b[0] - b[3] / 2; t.x2 = b[0] + b[3] / 2; t.y1 = b[1] - b[4] / 2; t.y2 = b[1] + b[4] / 2; t.z1 = 0.f; t.z2 = 0.f;
        t.ar = b[3] * b[4];
    } else {
        t.x1 = b[0]; t.y1 = b[1]; t.z1 = b[2]; t.x2 = b[3]; t.y2 = b[4]; t.z2 = b[5];
        t.ar = (b[3] - b[0]) * (b[4] - b[1]) * (b[5] - b[2]);
    }
    return t;
}

// does kept box a suppress box (bx1 .. bz2, sb)?
template <int MODE>
__device__ __forceinline__ bool nms_suppresses(const NmsTerms& a, float bx1, float bx2, float by1, float by2, float bz1, float bz2, float sb,
                                               float thr) {
    const float w = fmaxf(fminf(a.x2, bx2) - fmaxf(a.x1, bx1), 0.f), h = fmaxf(fminf(a.y2, by2) - fmaxf(a.y1, by1), 0.f);
    if (MODE == 0) {
        const float inter = w * h;
        const float iou = inter / fmaxf(a.ar + sb - inter, 1e-8f);
        return iou > thr;
    } else {
        const float d = fmaxf(fminf(a.z2, bz2) - fmaxf(a.z1, bz1), 0.f);
        const float inter = w * h * d;
        const float iou = inter / (a.ar + sb - inter);
        return !(iou <= thr);
    }
}

template <int MODE>
__global__ __launch_bounds__(1024) void nms_k(const float* __restrict__ boxes, const int32_t* __restrict__ labels, int n, float thr,
                                              uint8_t* __restrict__ keep) {
    extern __shared__ float sm[];
    float* x1 = sm; float* x2 = x1 + n; float* y1 = x2 + n; float* y2 = y1 + n; float* z1 = y2 + n; float* z2 = z1 + n; float* ar = z2 + n;
    int* lab = reinterpret_cast<int*>(ar + n);
    int* sup = lab + n;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const NmsTerms t = nms_terms<MODE>(boxes + i * 6);
        x1[i] = t.x1; x2[i] = t.x2; y1[i] = t.y1; y2[i] = t.y2; z1[i] = t.z1; z2[i] = t.z2; ar[i] = t.ar;
        lab[i] = labels[i]; sup[i] = 0;
        keep[i] = 0;
    }
    for (int i = 0; i < n; ++i) {
        __syncthreads();
        if (sup[i]) continue;                     // same LDS word for every thread: uniform
        if (threadIdx.x == 0) keep[i] = 1;
        const int li = lab[i];
        const NmsTerms a{x1[i], x2[i], y1[i], y2[i], z1[i], z2[i], ar[i]};
        for (int j = i + 1 + threadIdx.x; j < n; j += blockDim.x) {
            if (lab[j] != li) break;              // labels ascending: the class segment ended
            if (sup[j]) continue;
            if (nms_suppresses<MODE>(a, x1[j], x2[j], y1[j], y2[j], z1[j], z2[j], ar[j], thr)) sup[j] = 1;
        }
    }
}

// ---- rotated boxes: mmcv.ops.nms3d (unidet3d.py:626, with_yaw) -- greedy suppression by the BEV IoU of the rotated
// rectangles (x, y, dx, dy, heading).  The intersection area is summed edge by edge (no vertex sorting, no arrays): every
// edge of A is clipped to the inside of B (closed), every edge of B to the strict inside of A (so an edge shared by both
// outlines counts once), and a clipped piece P0->P1 of a counter-clockwise outline contributes cross(P0, P1) / 2.
__device__ __forceinline__ float clipped_edges_area(const float (&pa)[8], const float (&pb)[8], bool strict) {
    float area = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float px = pa[2 * e], py = pa[2 * e + 1];
        const float dx = pa[2 * ((e + 1) & 3)] - px, dy = pa[2 * ((e + 1) & 3) + 1] - py;
        float t0 = 0.f, t1 = 1.f;
        bool alive = true;
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            const float ax = pb[2 * f], ay = pb[2 * f + 1];
            const float ex = pb[2 * ((f + 1) & 3)] - ax, ey = pb[2 * ((f + 1) & 3) + 1] - ay;
            const float n0 = ex * (py - ay) - ey * (px - ax);       // side of the edge's start, > 0 = inside
            const float m = ex * dy - ey * dx;                       // change of the side along the edge
            if (m == 0.f) {
                // parallel: inside the half-plane, or -- for the closed test -- on f's line with the same direction (both
                // outlines on the same side, a true edge of the intersection).  Opposite directions are outlines that only touch
                // along the line, and a zero-length f (degenerate B) has no inside: neither contributes area.
                alive = alive && (strict ? n0 > 0.f : (n0 > 0.f || (n0 == 0.f && ex * dx + ey * dy > 0.f)));
            } else {
                const float tc = -n0 / m;
                if (m > 0.f) t0 = fmaxf(t0, tc); else t1 = fminf(t1, tc);
            }
        }
        if (alive && t0 < t1) {
            const float x0 = px + t0 * dx, y0 = py + t0 * dy, x1 = px + t1 * dx, y1 = py + t1 * dy;
            area += 0.5f * (x0 * y1 - x1 * y0);
        }
    }
    return area;
}

// corners (counter-clockwise) and BEV area of a rotated box (cx, cy, cz, dx, dy, dz, heading)
__device__ __forceinline__ float rot_corners(const float* b, float* cor) {
    const float c = cosf(b[6]), s = sinf(b[6]), hx = 0.5f * b[3], hy = 0.5f * b[4];
    const float sx[4] = {hx, -hx, -hx, hx}, sy[4] = {hy, hy, -hy, -hy};
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        cor[2 * v] = sx[v] * c - sy[v] * s + b[0];
        cor[2 * v + 1] = sx[v] * s + sy[v] * c + b[1];
    }
    return b[3] * b[4];
}

// does kept box i (corners relative to its first corner (ox, oy): pa, area sa) suppress the box with corners cj / area sb?
__device__ __forceinline__ bool rot_suppresses(const float (&pa)[8], float ox, float oy, float sa, const float* cj, float sb, float thr) {
    float pb[8];
#pragma unroll
    for (int v = 0; v < 4; ++v) { pb[2 * v] = cj[2 * v] - ox; pb[2 * v + 1] = cj[2 * v + 1] - oy; }
    const float inter = fmaxf(clipped_edges_area(pa, pb, false) + clipped_edges_area(pb, pa, true), 0.f);
    const float iou = inter / fmaxf(sa + sb - inter, 1e-8f);
    return iou > thr;
}

__device__ __forceinline__ void rot_relative(const float* ci, float (&pa)[8], float& ox, float& oy) {
    ox = ci[0]; oy = ci[1];                   // coordinates relative to a corner of box i
#pragma unroll
    for (int v = 0; v < 4; ++v) { pa[2 * v] = ci[2 * v] - ox; pa[2 * v + 1] = ci[2 * v + 1] - oy; }
}

__global__ __launch_bounds__(1024) void nms_rot_k(const float* __restrict__ boxes, const int32_t* __restrict__ labels, int n, float thr,
                                                  uint8_t* __restrict__ keep) {
    extern __shared__ float sm[];
    float* cor = sm;                     // [n][8] corners, counter-clockwise
    float* ar = cor + 8 * n;
    int* lab = reinterpret_cast<int*>(ar + n);
    int* sup = lab + n;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        ar[i] = rot_corners(boxes + i * 7, cor + i * 8);
        lab[i] = labels[i]; sup[i] = 0;
        keep[i] = 0;
    }
    for (int i = 0; i < n; ++i) {
        __syncthreads();
        if (sup[i]) continue;
        if (threadIdx.x == 0) keep[i] = 1;
        const int li = lab[i];
        float pa[8], ox, oy;
        rot_relative(cor + i * 8, pa, ox, oy);
        const float sa = ar[i];
        for (int j = i + 1 + threadIdx.x; j < n; j += blockDim.x) {
            if (lab[j] != li) break;
            if (sup[j]) continue;
            if (rot_suppresses(pa, ox, oy, sa, cor + j * 8, ar[j], thr)) sup[j] = 1;
        }
    }
}

// float min / max by integer atomics on the bit pattern: sign bit clear -> signed compare, set -> unsigned compare reversed.  The
// branch tests the sign bit, not v >= 0: -0.0f has it set (as a signed int it is INT_MIN, which would never raise a max and
// would overwrite a negative min).
__device__ __forceinline__ void atomic_min_f32(float* addr, float v) {
    if (__float_as_int(v) >= 0) atomicMin(reinterpret_cast<int*>(addr), __float_as_int(v));
    else atomicMax(reinterpret_cast<unsigned int*>(addr), __float_as_uint(v));
}
__device__ __forceinline__ void atomic_max_f32(float* addr, float v) {
    if (__float_as_int(v) >= 0) atomicMax(reinterpret_cast<int*>(addr), __float_as_int(v));
    else atomicMin(reinterpret_cast<unsigned int*>(addr), __float_as_uint(v));
}

__global__ void trim_init_k(float* __restrict__ mm, int nb) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nb * 6) mm[i] = (i % 6) < 3 ? INFINITY : -INFINITY;
}

// trimming of ONE box by ONE superpoint (points list[o0 .. o1) of the CSR): the inside ratio, then the delete / add rule applied to
// the box's (min xyz, max xyz) accumulator `out` by float atomics on the bit patterns (order-independent: min / max).  trim_k (one
// scene) and trim_seg_k (batched) both call it.
__device__ __forceinline__ void trim_one(const float* __restrict__ points, int64_t ld, const int32_t* __restrict__ list, int o0, int o1,
                                         const float* __restrict__ box, bool rot, float low, float up, float* __restrict__ out) {
    const float cx = box[0], cy = box[1], cz = box[2];
    const float hx = box[3] / 2, hy = box[4] / 2, hz = box[5] / 2;
    // heading (7-dof boxes): the shift p - c is rotated by -yaw about z before the face test (get_face_distances :666-668,
    // mmdet3d rotation_3d_in_axis: x' = x cos a - y sin a, y' = x sin a + y cos a with a = -yaw)
    float rs = 0.f, rc = 1.f;
    if (rot) { rs = sinf(-box[6]); rc = cosf(-box[6]); }
    float imin[3] = {INFINITY, INFINITY, INFINITY}, imax[3] = {-INFINITY, -INFINITY, -INFINITY};     // inside points
    float amin[3] = {INFINITY, INFINITY, INFINITY}, amax[3] = {-INFINITY, -INFINITY, -INFINITY};     // all points of s
    int cnt_in = 0;
    for (int o = o0; o < o1; ++o) {
        const float* p = points + (int64_t)list[o] * ld;
        const float px = p[0], py = p[1], pz = p[2];
        // get_face_distances with yaw 0: shift = p - c; centre' = c + shift; distances to the six faces
        float sx = px - cx, sy = py - cy;
        if (rot) { const float tx = sx * rc - sy * rs; sy = sx * rs + sy * rc; sx = tx; }
        const float ex = cx + sx, ey = cy + sy, ez = cz + (pz - cz);
        const bool in = ((ex - cx) + hx > 0.f) && ((cx + hx) - ex > 0.f) && ((ey - cy) + hy > 0.f) && ((cy + hy) - ey > 0.f) &&
                        ((ez - cz) + hz > 0.f) && ((cz + hz) - ez > 0.f);
        amin[0] = fminf(amin[0], px); amin[1] = fminf(amin[1], py); amin[2] = fminf(amin[2], pz);
        amax[0] = fmaxf(amax[0], px); amax[1] = fmaxf(amax[1], py); amax[2] = fmaxf(amax[2], pz);
        if (in) {
            ++cnt_in;
            imin[0] = fminf(imin[0], px); imin[1] = fminf(imin[1], py); imin[2] = fminf(imin[2], pz);
            imax[0] = fmaxf(imax[0], px); imax[1] = fmaxf(imax[1], py); imax[2] = fmaxf(imax[2], pz);
        }
    }
    const float ratio = (float)cnt_in / (float)(o1 - o0);      // scatter_mean of the 0/1 inside flags
    const bool add = ratio > up, del = ratio < low;            // :574-578: delete first, then add
    if (!add && (del || cnt_in == 0)) return;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        atomic_min_f32(out + d, add ? amin[d] : imin[d]);
        atomic_max_f32(out + 3 + d, add ? amax[d] : imax[d]);
    }
}

// one wave per (superpoint s, tile of 64 boxes): lane = box.  The superpoint's points are contiguous in the CSR list,
// so the wave knows the inside ratio of (box, s) after one pass and can apply the delete / add rule right away.
__global__ __launch_bounds__(64) void trim_k(const float* __restrict__ points, int64_t ld, const int32_t* __restrict__ list,
                                             const int32_t* __restrict__ offsets, int nbt, const float* __restrict__ boxes, int nb,
                                             int box_dim, float low, float up, float* __restrict__ mm) {
    const int s = blockIdx.x / nbt, b = (blockIdx.x % nbt) * 64 + threadIdx.x;
    const int o0 = offsets[s], o1 = offsets[s + 1];
    if (o0 >= o1 || b >= nb) return;
    trim_one(points, ld, list, o0, o1, boxes + b * box_dim, box_dim == 7, low, up, mm + b * 6);
}

// =====================================================================================================================
// Batched post-processing: every scene of a batch in one chain of launches, no host read in between (u3d.h "batched").
//   topk_seg_k   one workgroup per scene: radix-select of the k-th probability (uint32 bit patterns of non-negative floats
//                order like the values), collection of the elements above it plus the lowest-index ties, bitonic sort on
//                (score desc, flat index asc) in LDS;
//   nms_order_k  one workgroup per scene: drop score <= score_thr, stable sort by label (bitonic on (label, rank)), gather the
//                boxes in that order, (scene, class) segment table;
//   nms_seg_k    one workgroup per (class, scene): greedy suppression inside the segment (nms_suppresses / rot_suppresses);
//   compact_k    one workgroup per scene: index-ordered scan of the keep flags -> survivors in (label asc, score desc);
//   trim_seg_k   one wave per (superpoint, box-tile stride) of the trimmed scenes: trim_one against the scene's own boxes;
//   trim_finish_k  (centre, size) from the (min, max) accumulators.
constexpr int PP_SORT = 4096;          // bitonic sort size in LDS (32 KB of 64-bit keys)
constexpr int PP_MAX_K = NMS_ROT_MAX;  // candidates per scene: a class segment of rotated boxes must fit one workgroup's LDS
constexpr int PP_META = U3D_PP_META, PP_FMETA = U3D_PP_FMETA;
constexpr int PP_THREADS = 1024;

// exclusive prefix count of a 0/1 flag over the workgroup (blockDim.x a multiple of 64); `total` = the workgroup's count.
// wsum: LDS words, one per wave.  Every thread must call it (it holds two barriers).
__device__ __forceinline__ int block_excl_scan(bool f, int* wsum, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const unsigned long long m = __ballot(f);
    const int pre = __popcll(m & ((1ull << lane) - 1ull));
    __syncthreads();                                   // the previous call's readers are done with wsum
    if (lane == 0) wsum[w] = __popcll(m);
    __syncthreads();
    int off = 0, tot = 0;
    for (int i = 0; i < nw; ++i) {
        const int v = wsum[i];
        off += i < w ? v : 0;
        tot += v;
    }
    total = tot;
    return off + pre;
}

// ascending bitonic sort of keys[0 .. n2), n2 a power of two <= PP_SORT
__device__ __forceinline__ void bitonic_sort_u64(unsigned long long* keys, int n2) {
    for (int size = 2; size <= n2; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int i = threadIdx.x; i < (n2 >> 1); i += blockDim.x) {
                const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                const bool asc = (lo & size) == 0;
                const unsigned long long a = keys[lo], b = keys[hi];
                if ((a > b) == asc) { keys[lo] = b; keys[hi] = a; }
            }
        }
    }
    __syncthreads();
}

__device__ __forceinline__ int pow2_at_least(int n) {
    int p = 2;
    while (p < n) p <<= 1;
    return p;
}

__global__ __launch_bounds__(PP_THREADS) void topk_seg_k(const uint64_t* __restrict__ prob_ptrs, const int32_t* __restrict__ meta, int K,
                                                         float* __restrict__ score, int32_t* __restrict__ label, int32_t* __restrict__ query,
                                                         int32_t* __restrict__ count) {
    __shared__ unsigned long long keys[PP_SORT];
    __shared__ unsigned hist[256];
    __shared__ int wsum[PP_THREADS / 64];
    __shared__ unsigned sh_prefix;
    __shared__ int sh_remaining, sh_ngt;
    const int b = blockIdx.x;
    const int* m = meta + (int64_t)b * PP_META;
    const unsigned n = (unsigned)m[0], C = (unsigned)m[1], ld = (unsigned)m[2];
    const unsigned N = n * C;                                     // < 2^31 (checked by the host)
    const int take = (int)min((unsigned)min(m[3], K), N);
    if (threadIdx.x == 0) count[b] = take;
    if (take <= 0) return;                                        // uniform
    const float* P = reinterpret_cast<const float*>(prob_ptrs[b]);
    auto bits = [&](unsigned e) -> unsigned {
        const unsigned r = e / C;
        return __float_as_uint(P[(size_t)r * ld + (e - r * C)]);
    };
    // ---- radix select (8-bit digits, most significant first): the k-th largest bit pattern T and how many of the elements
    // equal to T belong to the top k (the elements above T all do)
    unsigned prefix = 0;
    int remaining = take;
    const bool all = (unsigned)take == N;
    if (!all) {
        for (int shift = 24; shift >= 0; shift -= 8) {
            const unsigned hi_mask = shift == 24 ? 0u : (~0u << (shift + 8));
            for (int i = threadIdx.x; i < 256; i += blockDim.x) hist[i] = 0;
            __syncthreads();
            for (unsigned e = threadIdx.x; e < N; e += blockDim.x) {
                const unsigned u = bits(e);
                if ((u & hi_mask) == prefix) atomicAdd(&hist[(u >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                int cum = 0, d = 255;
                for (; d > 0; --d) {
                    if (cum + (int)hist[d] >= remaining) break;
                    cum += (int)hist[d];
                }
                sh_prefix = prefix | ((unsigned)d << shift);
                sh_remaining = remaining - cum;
            }
            __syncthreads();
            prefix = sh_prefix;
            remaining = sh_remaining;
        }
    }
    // ---- collect: every element above T (any order) at [0, take - remaining), the first `remaining` elements equal to T in
    // index order at [take - remaining, take)
    if (threadIdx.x == 0) sh_ngt = 0;
    __syncthreads();
    const int n_gt = take - remaining;
    int taken_eq = 0;
    for (unsigned base = 0; base < N; base += blockDim.x) {
        const unsigned e = base + threadIdx.x;
        const unsigned u = e < N ? bits(e) : 0u;
        const bool gt = e < N && (all || u > prefix), eq = e < N && !all && u == prefix;
        if (gt) {
            const int pos = atomicAdd(&sh_ngt, 1);
            if (pos < take) keys[pos] = ((unsigned long long)(~u) << 32) | e;     // always true: count(> T) = take - remaining
        }
        int tot;
        const int r = block_excl_scan(eq, wsum, tot);
        if (eq && taken_eq + r < remaining) keys[n_gt + taken_eq + r] = ((unsigned long long)(~u) << 32) | e;
        taken_eq += tot;
    }
    const int n2 = pow2_at_least(take);
    for (int i = take + threadIdx.x; i < n2; i += blockDim.x) keys[i] = ~0ull;
    bitonic_sort_u64(keys, n2);
    for (int r = threadIdx.x; r < take; r += blockDim.x) {
        const unsigned long long k = keys[r];
        const unsigned e = (unsigned)k;
        const int64_t o = (int64_t)b * K + r;
        score[o] = __uint_as_float(~(unsigned)(k >> 32));
        label[o] = (int32_t)(e % C);
        query[o] = (int32_t)(e / C);
    }
}

__global__ __launch_bounds__(PP_THREADS) void nms_order_k(const uint64_t* __restrict__ box_ptrs, const int32_t* __restrict__ meta,
                                                          const float* __restrict__ fmeta, int K, int max_classes,
                                                          const float* __restrict__ score, const int32_t* __restrict__ label,
                                                          const int32_t* __restrict__ query, const int32_t* __restrict__ count,
                                                          int32_t* __restrict__ order, int32_t* __restrict__ n_order, float* __restrict__ boxes_ord,
                                                          int32_t* __restrict__ seg) {
    __shared__ unsigned long long keys[PP_SORT];
    __shared__ int sh_n;
    const int b = blockIdx.x;
    const int cnt = min(count[b], K);
    const int bd = meta[(int64_t)b * PP_META + 4];
    const float thr = fmeta[(int64_t)b * PP_FMETA + 0];
    int32_t* sg = seg + (int64_t)b * max_classes * 2;
    for (int c = threadIdx.x; c < 2 * max_classes; c += blockDim.x) sg[c] = 0;
    if (threadIdx.x == 0) sh_n = 0;
    const int n2 = pow2_at_least(cnt);
    __syncthreads();
    for (int r = threadIdx.x; r < n2; r += blockDim.x) {
        const int64_t o = (int64_t)b * K + r;
        const bool ok = r < cnt && score[o] > thr;
        keys[r] = ok ? (((unsigned long long)(unsigned)label[o] << 32) | (unsigned)r) : ~0ull;
        if (ok) atomicAdd(&sh_n, 1);
    }
    bitonic_sort_u64(keys, n2);             // (label asc, rank asc) = torch.sort(labels, stable=True) of the score-sorted list
    const int n = sh_n;
    if (threadIdx.x == 0) n_order[b] = n;
    const float* B0 = reinterpret_cast<const float*>(box_ptrs[b]);
    for (int p = threadIdx.x; p < n; p += blockDim.x) {
        const unsigned long long k = keys[p];
        const int r = (int)(unsigned)k, l = (int)(k >> 32);
        const int64_t o = (int64_t)b * K + p;
        order[o] = r;
        const float* src = B0 + (int64_t)query[(int64_t)b * K + r] * bd;
        float* dst = boxes_ord + o * 7;
#pragma unroll
        for (int d = 0; d < 6; ++d) dst[d] = src[d];
        dst[6] = bd == 7 ? src[6] : 0.f;
        if (l >= max_classes) continue;                            // (the caller guarantees max_classes >= every C)
        if (p == 0 || (int)(keys[p - 1] >> 32) != l) sg[2 * l] = p;
        if (p == n - 1 || (int)(keys[p + 1] >> 32) != l) sg[2 * l + 1] = p + 1;
    }
}

// greedy suppression over one class segment [s0, s0 + n) of scene b: the loops of nms_k / nms_rot_k without the label test
template <int MODE>
__device__ __forceinline__ void nms_segment(const float* __restrict__ bx, int n, float thr, uint8_t* __restrict__ keep, float* sm) {
    float* x1 = sm; float* x2 = x1 + n; float* y1 = x2 + n; float* y2 = y1 + n; float* z1 = y2 + n; float* z2 = z1 + n; float* ar = z2 + n;
    int* sup = reinterpret_cast<int*>(ar + n);
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const float* b = bx + i * 7;
        float c6[6];
        if (MODE == 1) {                       // _bbox_to_loss: (centre, size) -> corners, as ops.nms_multiclass does it
#pragma unroll
            for (int d = 0; d < 3; ++d) { c6[d] = b[d] - b[3 + d] / 2; c6[3 + d] = b[d] + b[3 + d] / 2; }
        }
        const NmsTerms t = nms_terms<MODE>(MODE == 1 ? c6 : b);
        x1[i] = t.x1; x2[i] = t.x2; y1[i] = t.y1; y2[i] = t.y2; z1[i] = t.z1; z2[i] = t.z2; ar[i] = t.ar;
        sup[i] = 0;
        keep[i] = 0;
    }
    for (int i = 0; i < n; ++i) {
        __syncthreads();
        if (sup[i]) continue;
        if (threadIdx.x == 0) keep[i] = 1;
        const NmsTerms a{x1[i], x2[i], y1[i], y2[i], z1[i], z2[i], ar[i]};
        for (int j = i + 1 + threadIdx.x; j < n; j += blockDim.x) {
            if (sup[j]) continue;
            if (nms_suppresses<MODE>(a, x1[j], x2[j], y1[j], y2[j], z1[j], z2[j], ar[j], thr)) sup[j] = 1;
        }
    }
}

__device__ __forceinline__ void nms_segment_rot(const float* __restrict__ bx, int n, float thr, uint8_t* __restrict__ keep, float* sm) {
    float* cor = sm;
    float* ar = cor + 8 * n;
    int* sup = reinterpret_cast<int*>(ar + n);
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        ar[i] = rot_corners(bx + i * 7, cor + i * 8);
        sup[i] = 0;
        keep[i] = 0;
    }
    for (int i = 0; i < n; ++i) {
        __syncthreads();
        if (sup[i]) continue;
        if (threadIdx.x == 0) keep[i] = 1;
        float pa[8], ox, oy;
        rot_relative(cor + i * 8, pa, ox, oy);
        const float sa = ar[i];
        for (int j = i + 1 + threadIdx.x; j < n; j += blockDim.x) {
            if (sup[j]) continue;
            if (rot_suppresses(pa, ox, oy, sa, cor + j * 8, ar[j], thr)) sup[j] = 1;
        }
    }
}

constexpr int PP_NMS_THREADS = 256;

__global__ __launch_bounds__(PP_NMS_THREADS) void nms_seg_k(const int32_t* __restrict__ meta, const float* __restrict__ fmeta, int K,
                                                            int max_classes, const int32_t* __restrict__ seg, const float* __restrict__ boxes_ord,
                                                            uint8_t* __restrict__ keep) {
    extern __shared__ float sm[];
    const int c = blockIdx.x, b = blockIdx.y;
    const int32_t* sg = seg + ((int64_t)b * max_classes + c) * 2;
    const int s0 = sg[0], n = sg[1] - sg[0];
    if (n <= 0) return;                                            // empty segment (uniform)
    const int mode = meta[(int64_t)b * PP_META + 5];
    const float thr = fmeta[(int64_t)b * PP_FMETA + 1];
    const float* bx = boxes_ord + ((int64_t)b * K + s0) * 7;
    uint8_t* kp = keep + (int64_t)b * K + s0;
    if (mode == 0) nms_segment<0>(bx, n, thr, kp, sm);
    else if (mode == 1) nms_segment<1>(bx, n, thr, kp, sm);
    else nms_segment_rot(bx, n, thr, kp, sm);
}

__global__ __launch_bounds__(PP_THREADS) void compact_k(const int32_t* __restrict__ meta, int K, const float* __restrict__ score,
                                                        const int32_t* __restrict__ label, const int32_t* __restrict__ order,
                                                        const int32_t* __restrict__ n_order, const uint8_t* __restrict__ keep,
                                                        const float* __restrict__ boxes_ord, float* __restrict__ out_boxes,
                                                        float* __restrict__ out_scores, int64_t* __restrict__ out_labels,
                                                        int32_t* __restrict__ out_count, int32_t* __restrict__ yaw, float* __restrict__ minmax) {
    __shared__ int wsum[PP_THREADS / 64];
    __shared__ int sh_yaw;
    const int b = blockIdx.x;
    const int n = n_order[b];
    const bool trim = meta[(int64_t)b * PP_META + 6] != 0;
    if (threadIdx.x == 0) sh_yaw = 0;
    int base = 0;
    for (int p0 = 0; p0 < n; p0 += blockDim.x) {
        const int p = p0 + threadIdx.x;
        const int64_t ip = (int64_t)b * K + p;
        const bool f = p < n && keep[ip];
        int tot;
        const int r = block_excl_scan(f, wsum, tot);
        if (f) {
            const int64_t o = (int64_t)b * K + base + r, src = (int64_t)b * K + order[ip];
            const float* bi = boxes_ord + ip * 7;
            float* bo = out_boxes + o * 7;
#pragma unroll
            for (int d = 0; d < 7; ++d) bo[d] = bi[d];
            if (bi[6] != 0.f) sh_yaw = 1;                       // ops.py: (bboxes[:, 6] != 0).any() (NaN counts as a heading)
            out_scores[o] = score[src];
            out_labels[o] = label[src];
            if (trim) {
#pragma unroll
                for (int d = 0; d < 6; ++d) minmax[o * 6 + d] = d < 3 ? INFINITY : -INFINITY;
            }
        }
        base += tot;
    }
    __syncthreads();
    if (threadIdx.x == 0) { out_count[b] = base; yaw[b] = sh_yaw; }
}

constexpr int PP_TRIM_TILES = 4;       // box tiles of 64 per superpoint handled by separate waves (the rest strided)

__global__ __launch_bounds__(64) void trim_seg_k(const float* __restrict__ points, int64_t ld, const int32_t* __restrict__ list,
                                                 const int32_t* __restrict__ offsets, const int32_t* __restrict__ sp_scene, int B,
                                                 const int32_t* __restrict__ meta, const float* __restrict__ fmeta, int K,
                                                 const int32_t* __restrict__ count, const int32_t* __restrict__ yaw,
                                                 const float* __restrict__ boxes, float* __restrict__ minmax) {
    const int s = blockIdx.x;
    int b = 0;
    while (b + 1 < B && sp_scene[b + 1] <= s) ++b;
    if (meta[(int64_t)b * PP_META + 6] == 0) return;
    const int o0 = offsets[s], o1 = offsets[s + 1], nb = count[b];
    if (o0 >= o1) return;
    const float low = fmeta[(int64_t)b * PP_FMETA + 2], up = fmeta[(int64_t)b * PP_FMETA + 3];
    const bool rot = yaw[b] != 0;
    for (int t = blockIdx.y * 64; t < nb; t += gridDim.y * 64) {
        const int i = t + threadIdx.x;
        if (i < nb) {
            const int64_t o = (int64_t)b * K + i;
            trim_one(points, ld, list, o0, o1, boxes + o * 7, rot, low, up, minmax + o * 6);
        }
    }
}

__global__ void trim_finish_k(const int32_t* __restrict__ meta, int K, const int32_t* __restrict__ count, const float* __restrict__ minmax,
                              float* __restrict__ boxes) {
    const int b = blockIdx.y;
    if (meta[(int64_t)b * PP_META + 6] == 0) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count[b]) return;
    const int64_t o = (int64_t)b * K + i;
    const float* mm = minmax + o * 6;
    float* bo = boxes + o * 7;
#pragma unroll
    for (int d = 0; d < 3; ++d) {                                   // ops.trim_boxes_by_superpoints: ((mx + mn) / 2, mx - mn)
        bo[d] = (mm[3 + d] + mm[d]) / 2;
        bo[3 + d] = mm[3 + d] - mm[d];
    }
}

}  // namespace u3d

using namespace u3d;

extern "C" {

// a launch that wants more than 64 KB of dynamic LDS has to raise the kernel's limit first (gfx950: 160 KB per workgroup)
static int lds_opt_in(const void* kernel, size_t bytes) {
    if (bytes <= 64 * 1024) return U3D_OK;
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) {
        (void)hipGetLastError();
        set_error("nms: cannot reserve %zu bytes of LDS", bytes);
        return U3D_EUNSUPPORTED;
    }
    return U3D_OK;
}

static int launch_nms(int mode, const float* boxes, const int32_t* labels, int n, float iou_thr, uint8_t* keep, u3d_stream_t stream) {
    if (n < 0 || (n > 0 && (!boxes || !labels || !keep))) return U3D_EINVAL;
    if (n == 0) return U3D_OK;
    if (n > NMS_MAX) {
        set_error("nms: %d boxes exceed the single-workgroup limit of %d", n, NMS_MAX);
        return U3D_EUNSUPPORTED;
    }
    const size_t lds = (size_t)n * 9 * sizeof(float);
    if (int rc = lds_opt_in(mode == 0 ? (const void*)nms_k<0> : (const void*)nms_k<1>, lds)) return rc;
    if (mode == 0) hipLaunchKernelGGL(nms_k<0>, dim3(1), dim3(1024), lds, (hipStream_t)stream, boxes, labels, n, iou_thr, keep);
    else hipLaunchKernelGGL(nms_k<1>, dim3(1), dim3(1024), lds, (hipStream_t)stream, boxes, labels, n, iou_thr, keep);
    return check_launch("nms");
}

int u3d_nms_bev(const float* boxes, const int32_t* labels, int n, float iou_thr, uint8_t* keep, u3d_stream_t stream) {
    return launch_nms(0, boxes, labels, n, iou_thr, keep, stream);
}

int u3d_nms_rotated(const float* boxes, const int32_t* labels, int n, float iou_thr, uint8_t* keep, u3d_stream_t stream) {
    if (n < 0 || (n > 0 && (!boxes || !labels || !keep))) return U3D_EINVAL;
    if (n == 0) return U3D_OK;
    if (n > NMS_ROT_MAX) {
        set_error("nms_rotated: %d boxes exceed the single-workgroup limit of %d", n, NMS_ROT_MAX);
        return U3D_EUNSUPPORTED;
    }
    if (int rc = lds_opt_in((const void*)nms_rot_k, (size_t)n * 11 * sizeof(float))) return rc;
    hipLaunchKernelGGL(nms_rot_k, dim3(1), dim3(1024), (size_t)n * 11 * sizeof(float), (hipStream_t)stream, boxes, labels, n, iou_thr, keep);
    return check_launch("nms_rotated");
}

int u3d_nms_aligned3d(const float* corners, const int32_t* labels, int n, float iou_thr, uint8_t* keep, u3d_stream_t stream) {
    return launch_nms(1, corners, labels, n, iou_thr, keep, stream);
}

int u3d_trim_boxes(const float* points, int64_t pt_ld, const int32_t* sp_list, const int32_t* sp_offsets, int S,
                   const float* boxes, int nb, int box_dim, float low_thr, float up_thr, float* minmax, u3d_stream_t stream) {
    if (nb < 0 || S < 0 || pt_ld < 3 || (box_dim != 6 && box_dim != 7) || (nb > 0 && (!boxes || !minmax)) || (S > 0 && (!points || !sp_list || !sp_offsets))) return U3D_EINVAL;
    if (nb == 0) return U3D_OK;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(trim_init_k, dim3((unsigned)ceil_div(nb * 6, 256)), dim3(256), 0, s, minmax, nb);
    if (S > 0) {
        const int nbt = (int)ceil_div(nb, 64);
        hipLaunchKernelGGL(trim_k, dim3((unsigned)((int64_t)S * nbt)), dim3(64), 0, s, points, pt_ld, sp_list, sp_offsets, nbt, boxes, nb, box_dim,
                           low_thr, up_thr, minmax);
    }
    return check_launch("trim_boxes");
}

// ---- batched post-processing ---------------------------------------------------------------------------------------------
int u3d_topk_segmented(const uint64_t* prob_ptrs, const int32_t* meta, int B, int K, float* score, int32_t* label, int32_t* query,
                       int32_t* count, u3d_stream_t stream) {
    if (B < 0 || K < 1 || K > PP_MAX_K || (B > 0 && (!prob_ptrs || !meta || !score || !label || !query || !count))) return U3D_EINVAL;
    if (B == 0) return U3D_OK;
    hipLaunchKernelGGL(topk_seg_k, dim3(B), dim3(PP_THREADS), 0, (hipStream_t)stream, prob_ptrs, meta, K, score, label, query, count);
    return check_launch("topk_segmented");
}

int64_t u3d_nms_batched_ws_bytes(int B, int max_classes) {
    return (int64_t)(B > 0 ? B : 0) * (max_classes > 0 ? max_classes : 0) * 2 * (int64_t)sizeof(int32_t) + 256;
}

int u3d_nms_batched(const uint64_t* box_ptrs, const int32_t* meta, const float* fmeta, int B, int K, int max_classes, const float* score,
                    const int32_t* label, const int32_t* query, const int32_t* count, int32_t* order, int32_t* n_order, uint8_t* keep,
                    float* boxes_ord, void* ws, u3d_stream_t stream) {
    if (B < 0 || K < 1 || K > PP_MAX_K || max_classes < 1 || max_classes > 65535) return U3D_EINVAL;
    if (B > 0 && (!box_ptrs || !meta || !fmeta || !score || !label || !query || !count || !order || !n_order || !keep || !boxes_ord || !ws))
        return U3D_EINVAL;
    if (B == 0) return U3D_OK;
    hipStream_t s = (hipStream_t)stream;
    int32_t* seg = static_cast<int32_t*>(ws);
    hipLaunchKernelGGL(nms_order_k, dim3(B), dim3(PP_THREADS), 0, s, box_ptrs, meta, fmeta, K, max_classes, score, label, query, count,
                       order, n_order, boxes_ord, seg);
    const size_t lds = (size_t)K * 10 * sizeof(float);            // rotated segments: 8 corner words + area + flag per box
    if (int rc = lds_opt_in((const void*)nms_seg_k, lds)) return rc;
    hipLaunchKernelGGL(nms_seg_k, dim3(max_classes, B), dim3(PP_NMS_THREADS), lds, s, meta, fmeta, K, max_classes, seg, boxes_ord, keep);
    return check_launch("nms_batched");
}

int u3d_nms_compact(const int32_t* meta, int B, int K, const float* score, const int32_t* label, const int32_t* order, const int32_t* n_order,
                    const uint8_t* keep, const float* boxes_ord, float* out_boxes, float* out_scores, int64_t* out_labels, int32_t* out_count,
                    int32_t* yaw, float* minmax, u3d_stream_t stream) {
    if (B < 0 || K < 1) return U3D_EINVAL;
    if (B > 0 && (!meta || !score || !label || !order || !n_order || !keep || !boxes_ord || !out_boxes || !out_scores || !out_labels ||
                  !out_count || !yaw || !minmax))
        return U3D_EINVAL;
    if (B == 0) return U3D_OK;
    hipLaunchKernelGGL(compact_k, dim3(B), dim3(PP_THREADS), 0, (hipStream_t)stream, meta, K, score, label, order, n_order, keep, boxes_ord,
                       out_boxes, out_scores, out_labels, out_count, yaw, minmax);
    return check_launch("nms_compact");
}

int u3d_trim_boxes_batched(const float* points, int64_t pt_ld, const int32_t* sp_list, const int32_t* sp_offsets, const int32_t* sp_scene,
                           int B, int S, const int32_t* meta, const float* fmeta, int K, const int32_t* count, const int32_t* yaw,
                           float* minmax, float* boxes, u3d_stream_t stream) {
    if (B < 0 || S < 0 || K < 1 || pt_ld < 3) return U3D_EINVAL;
    if (B > 0 && (!meta || !fmeta || !count || !yaw || !minmax || !boxes || !sp_scene)) return U3D_EINVAL;
    if (S > 0 && (!points || !sp_list || !sp_offsets)) return U3D_EINVAL;
    if (B == 0) return U3D_OK;
    hipStream_t s = (hipStream_t)stream;
    if (S > 0) {
        const int tiles = (int)(ceil_div(K, 64) < PP_TRIM_TILES ? ceil_div(K, 64) : PP_TRIM_TILES);
        hipLaunchKernelGGL(trim_seg_k, dim3(S, tiles), dim3(64), 0, s, points, pt_ld, sp_list, sp_offsets, sp_scene, B, meta, fmeta, K, count,
                           yaw, boxes, minmax);
    }
    hipLaunchKernelGGL(trim_finish_k, dim3((unsigned)ceil_div(K, 256), B), dim3(256), 0, s, meta, K, count, minmax, boxes);
    return check_launch("trim_boxes_batched");
}

}  // extern "C"
