// Detection evaluation (mAP / mAR at IoU thresholds) of one dataset's whole validation pass on the device (include/u3d.h, "R16"):
// the arithmetic of evaluation.indoor_eval / eval_det_cls / average_precision without a host loop.
//
// Input: every detection and ground truth of the pass packed image after image ([D][7] / [G][7] bottom-centre depth boxes, labels,
// CSR offsets per image).  Three entry points, a fixed chain of launches:
//   u3d_eval_match   per detection the best same-class ground truth of its image (first maximum of a strict '>' scan in
//                    ground-truth order) + class histograms.  One thread per detection; a workgroup covers 256 consecutive
//                    detections, walks the images they belong to and stages each image's ground truths through LDS in chunks of
//                    EV_GT_CHUNK boxes (an image may have more).
//   u3d_eval_order   keys (class << 32 | order-preserving uint of -score) + one stable u3d_sort_u64: class ascending, score
//                    descending, ties by packed index.
//   u3d_eval_sweep   the greedy true-positive assignment and the precision / recall curves of every (class, threshold).
//
// Why the greedy sweep is parallel: eval_det_cls marks detection d (in sorted order) a true positive iff iou_max[d] > thr and the
// ground truth jmax[d] has not been taken -- and only a detection that passes the SAME test on the SAME ground truth can have
// taken it (a detection never falls back to its second-best ground truth).  So d is a true positive iff it is the first one, in
// sorted order, among the detections with iou_max > thr that name jmax[d]: an integer atomicMin of the sorted rank per (ground
// truth, threshold).  Integer min does not depend on arrival order, so the result is bit-reproducible.
//
// The curves: one workgroup per (class, threshold) walks its segment of the sorted order in tiles of 1024 with a carry -- forward for
// the cumulative true-positive count (integers), backward for the precision envelope (a reverse running maximum: exact in any
// order) and the area sum over the points where recall changes (the true positives), fp64, fixed order.  tp + fp at position k of a
// segment is k + 1, so precision = tp / (k + 1) and recall = tp / npos are the host's fp64 quotients bit for bit.
//
// Axis-aligned pairs (both headings exactly 0) use evaluation.boxes_iou_3d's fp32 expression in its operation order (compiled with
// -ffp-contract=off: bit-equal); any other pair intersects the two rectangles in the detection's own frame in fp64 (edges of one
// clipped to the other, as in postproc.hip; in that frame a pair with a common heading has exactly parallel edges).
#include <math.h>

#include "u3d_common.h"

namespace u3d {

constexpr int EV_THREADS = 256;
constexpr int EV_GT_CHUNK = U3D_EVAL_GT_CHUNK;    // ground truths of an image staged in LDS at a time
constexpr int EV_ITEMS = 4;                        // consecutive positions of a segment per thread
constexpr int EV_TILE = EV_THREADS * EV_ITEMS;
constexpr int EV_MAX_T = U3D_EVAL_MAX_THR;
constexpr int EV_MAX_C = U3D_EVAL_MAX_CLASSES;

struct EvalThr { float v[EV_MAX_T]; };

// ---- class histograms (integer atomics: order-free) ----
__global__ __launch_bounds__(EV_THREADS) void eval_count_k(const int32_t* __restrict__ labels, int64_t n, int C, int32_t* __restrict__ counts) {
    __shared__ int32_t h[EV_MAX_C];
    for (int c = threadIdx.x; c < C; c += EV_THREADS) h[c] = 0;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * EV_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * EV_THREADS) {
        const int l = labels[i];
        if ((unsigned)l < (unsigned)C) atomicAdd(&h[l], 1);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += EV_THREADS)
        if (h[c]) atomicAdd(&counts[c], h[c]);
}

// ---- IoU of two bottom-centre boxes (x, y, z_bottom, dx, dy, dz, yaw) ----
__device__ __forceinline__ float iou_aligned(const float (&a)[7], const float* b) {
    const float zlo = fmaxf(a[2], b[2]), zhi = fminf(a[2] + a[5], b[2] + b[5]);
    const float h = fmaxf(zhi - zlo, 0.f);
    const float wx = fmaxf(fminf(a[0] + a[3] / 2, b[0] + b[3] / 2) - fmaxf(a[0] - a[3] / 2, b[0] - b[3] / 2), 0.f);
    const float wy = fmaxf(fminf(a[1] + a[4] / 2, b[1] + b[4] / 2) - fmaxf(a[1] - a[4] / 2, b[1] - b[4] / 2), 0.f);
    const float bev = wx * wy;
    const float inter = bev * h;
    const float v1 = a[3] * a[4] * a[5], v2 = b[3] * b[4] * b[5];
    return inter / fmaxf(v1 + v2 - inter, 1e-8f);
}

// area of the part of outline pa (counter-clockwise) that lies inside pb: every edge of pa clipped to the four half-planes of pb
// (closed, or strict so that an edge shared by both outlines counts once); a piece P0 -> P1 contributes cross(P0, P1) / 2
__device__ __forceinline__ double clipped_edges_area(const double (&pa)[8], const double (&pb)[8], bool strict) {
    double area = 0.0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const double px = pa[2 * e], py = pa[2 * e + 1];
        const double dx = pa[2 * ((e + 1) & 3)] - px, dy = pa[2 * ((e + 1) & 3) + 1] - py;
        double t0 = 0.0, t1 = 1.0;
        bool alive = true;
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            const double ax = pb[2 * f], ay = pb[2 * f + 1];
            const double ex = pb[2 * ((f + 1) & 3)] - ax, ey = pb[2 * ((f + 1) & 3) + 1] - ay;
            const double n0 = ex * (py - ay) - ey * (px - ax);      // side of the edge's start, > 0 = inside
            const double m = ex * dy - ey * dx;                      // change of the side along the edge
            if (m == 0.0) {
                alive = alive && (strict ? n0 > 0.0 : (n0 > 0.0 || (n0 == 0.0 && ex * dx + ey * dy > 0.0)));
            } else {
                const double tc = -n0 / m;
                if (m > 0.0) t0 = fmax(t0, tc); else t1 = fmin(t1, tc);
            }
        }
        if (alive && t0 < t1) {
            const double x0 = px + t0 * dx, y0 = py + t0 * dy, x1 = px + t1 * dx, y1 = py + t1 * dy;
            area += 0.5 * (x0 * y1 - x1 * y0);
        }
    }
    return area;
}

// ca / sa: cosine / sine of a's heading (fp64)
__device__ __forceinline__ float iou_rotated(const float (&a)[7], double ca, double sa, const float* b) {
    const double hx = 0.5 * (double)a[3], hy = 0.5 * (double)a[4], gx = 0.5 * (double)b[3], gy = 0.5 * (double)b[4];
    const double da = (double)b[6] - (double)a[6];
    const double cb = cos(da), sb = sin(da);
    const double ox = (double)b[0] - (double)a[0], oy = (double)b[1] - (double)a[1];
    const double lx = ca * ox + sa * oy, ly = ca * oy - sa * ox;                 // b's centre in a's frame
    const double pa[8] = {hx, hy, -hx, hy, -hx, -hy, hx, -hy};
    const double qx[4] = {gx, -gx, -gx, gx}, qy[4] = {gy, gy, -gy, -gy};
    double pb[8];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        pb[2 * v] = qx[v] * cb - qy[v] * sb + lx;
        pb[2 * v + 1] = qx[v] * sb + qy[v] * cb + ly;
    }
    const double bev = fmax(clipped_edges_area(pa, pb, false) + clipped_edges_area(pb, pa, true), 0.0);
    const double zlo = fmax((double)a[2], (double)b[2]), zhi = fmin((double)a[2] + (double)a[5], (double)b[2] + (double)b[5]);
    const double inter = bev * fmax(zhi - zlo, 0.0);
    const double v1 = (double)a[3] * (double)a[4] * (double)a[5], v2 = (double)b[3] * (double)b[4] * (double)b[5];
    return (float)(inter / fmax(v1 + v2 - inter, 1e-8));
}

// last image i in [0, I) with off[i] <= d (offsets ascending, off[0] = 0): the image that owns packed row d
__device__ __forceinline__ int image_of(const int32_t* __restrict__ off, int I, int d) {
    int lo = 0, hi = I;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= d) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(EV_THREADS) void eval_match_k(const float* __restrict__ det_boxes, const int32_t* __restrict__ det_labels,
                                                           const int32_t* __restrict__ det_off, const float* __restrict__ gt_boxes,
                                                           const int32_t* __restrict__ gt_labels, const int32_t* __restrict__ gt_off, int D, int G,
                                                           int I, int C, float* __restrict__ iou_max, int32_t* __restrict__ jmax) {
    __shared__ uint32_t sb[EV_GT_CHUNK][8];      // box bits + label
    const int d_first = blockIdx.x * EV_THREADS, d = d_first + threadIdx.x;
    const int d_last = d_first + EV_THREADS - 1 < D - 1 ? d_first + EV_THREADS - 1 : D - 1;
    const bool have = d < D;
    float a[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int la = -1, img = -1;
    if (have) {
#pragma unroll
        for (int k = 0; k < 7; ++k) a[k] = det_boxes[(int64_t)d * 7 + k];
        la = det_labels[d];
        if ((unsigned)la >= (unsigned)C) la = -1;
        img = image_of(det_off, I, d);
    }
    const double ca = cos((double)a[6]), sa = sin((double)a[6]);
    const int img_lo = image_of(det_off, I, d_first), img_hi = image_of(det_off, I, d_last);     // block-uniform
    float best = -INFINITY;
    int jb = -1;
    for (int im = img_lo; im <= img_hi; ++im) {
        if (det_off[im + 1] <= det_off[im]) continue;                  // an image without detections lies between two others
        const int g0 = clampi(gt_off[im], 0, G), g1 = clampi(gt_off[im + 1], g0, G);
        for (int base = g0; base < g1; base += EV_GT_CHUNK) {
            const int n = g1 - base < EV_GT_CHUNK ? g1 - base : EV_GT_CHUNK;
            __syncthreads();                                           // the previous chunk has been read
            for (int e = threadIdx.x; e < n * 8; e += EV_THREADS) {
                const int j = e >> 3, k = e & 7;
                sb[j][k] = k < 7 ? __float_as_uint(gt_boxes[(int64_t)(base + j) * 7 + k]) : (uint32_t)gt_labels[base + j];
            }
            __syncthreads();
            if (have && img == im && la >= 0) {
                for (int j = 0; j < n; ++j) {
                    if ((int)sb[j][7] != la) continue;
                    float b[7];
#pragma unroll
                    for (int k = 0; k < 7; ++k) b[k] = __uint_as_float(sb[j][k]);
                    const float iou = (a[6] == 0.f && b[6] == 0.f) ? iou_aligned(a, b) : iou_rotated(a, ca, sa, b);
                    if (iou > best) { best = iou; jb = base + j; }
                }
            }
        }
    }
    if (have) { iou_max[d] = best; jmax[d] = jb; }
}

// ---- ordering keys: class << 32 | uint that ascends with -score (any finite score; -0 and +0 tie; NaN last, as numpy sorts it) ----
__global__ __launch_bounds__(EV_THREADS) void eval_keys_k(const float* __restrict__ scores, const int32_t* __restrict__ labels, int D, int C,
                                                          uint64_t* __restrict__ keys) {
    const int d = blockIdx.x * EV_THREADS + threadIdx.x;
    if (d >= D) return;
    float f = -scores[d];
    if (f == 0.f) f = 0.f;
    const uint32_t u = (uint32_t)__float_as_int(f);
    uint32_t o = (u >> 31) ? ~u : (u | 0x80000000u);
    if (f != f) o = 0xffffffffu;
    const int l = labels[d];
    const uint32_t cls = (unsigned)l < (unsigned)C ? (uint32_t)l : (uint32_t)C;      // labels outside [0, C) sort behind every class
    keys[d] = ((uint64_t)cls << 32) | o;
}

// ---- first claimant per (ground truth, threshold) ----
__global__ __launch_bounds__(EV_THREADS) void eval_claim_k(const float* __restrict__ iou_max, const int32_t* __restrict__ jmax,
                                                           const int32_t* __restrict__ perm, int D, int G, int T, EvalThr thr,
                                                           int32_t* __restrict__ claim) {
    const int r = blockIdx.x * EV_THREADS + threadIdx.x;
    if (r >= D) return;
    const int d = perm[r];
    if ((unsigned)d >= (unsigned)D) return;
    const int j = jmax[d];
    if ((unsigned)j >= (unsigned)G) return;
    const float iou = iou_max[d];
    for (int t = 0; t < T; ++t)
        if (iou > thr.v[t]) atomicMin(&claim[(int64_t)t * G + j], r);
}

__global__ __launch_bounds__(EV_THREADS) void eval_flag_k(const float* __restrict__ iou_max, const int32_t* __restrict__ jmax,
                                                          const int32_t* __restrict__ perm, int D, int G, int T, EvalThr thr,
                                                          const int32_t* __restrict__ claim, uint8_t* __restrict__ flag) {
    const int r = blockIdx.x * EV_THREADS + threadIdx.x;
    if (r >= D) return;
    const int d = perm[r];
    const bool ok = (unsigned)d < (unsigned)D;
    const int j = ok ? jmax[d] : -1;
    const bool okj = (unsigned)j < (unsigned)G;
    const float iou = ok ? iou_max[d] : -INFINITY;
    for (int t = 0; t < T; ++t)
        flag[(int64_t)t * D + r] = (okj && iou > thr.v[t] && claim[(int64_t)t * G + j] == r) ? 1 : 0;
}

// ---- workgroup scans through LDS (Hillis-Steele, fixed order).  reverse: thread EV_THREADS - 1 comes first.  Returns the inclusive
// value of the calling thread; excl = the value of its predecessor (identity for the first), total = the value of the last. ----
template <typename V, typename Op>
__device__ __forceinline__ V block_scan(V v, V identity, bool reverse, V* sh, Op op, V& excl, V& total) {
    const int p = reverse ? EV_THREADS - 1 - (int)threadIdx.x : (int)threadIdx.x;
    __syncthreads();                              // sh may still be read from the previous call
    sh[p] = v;
    __syncthreads();
    for (int off = 1; off < EV_THREADS; off <<= 1) {
        V x = sh[p];
        if (p >= off) x = op(sh[p - off], x);
        __syncthreads();
        sh[p] = x;
        __syncthreads();
    }
    excl = p > 0 ? sh[p - 1] : identity;
    total = sh[EV_THREADS - 1];
    return sh[p];
}

struct OpAddI { __device__ int operator()(int a, int b) const { return a + b; } };
struct OpAddD { __device__ double operator()(double a, double b) const { return a + b; } };
struct OpMaxD { __device__ double operator()(double a, double b) const { return fmax(a, b); } };

// one workgroup per (class, threshold)
__global__ __launch_bounds__(EV_THREADS) void eval_scan_k(const uint8_t* __restrict__ flag, const int32_t* __restrict__ n_gt,
                                                          const int32_t* __restrict__ n_det, int D, int C, float* __restrict__ ap,
                                                          float* __restrict__ rec, int32_t* __restrict__ cum) {
    __shared__ int shi[EV_THREADS];
    __shared__ double shd[EV_THREADS];
    const int c = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
    int part = 0;
    for (int k = tid; k < c; k += EV_THREADS) part += n_det[k];
    int ex_i, s0;
    block_scan<int>(part, 0, false, shi, OpAddI(), ex_i, s0);          // s0: first sorted rank of the class
    int nd = n_det[c];
    const int npos = n_gt[c];
    if (s0 < 0 || s0 > D) nd = 0;
    else if (nd > D - s0) nd = D - s0;
    const int64_t out = (int64_t)t * C + c;
    if (nd <= 0) {                                 // no detections: AP = recall = 0 (a class absent from both is not reported by the host)
        if (tid == 0) { ap[out] = 0.f; rec[out] = 0.f; }
        return;
    }
    const uint8_t* __restrict__ f = flag + (int64_t)t * D + s0;
    int32_t* __restrict__ cm = cum + (int64_t)t * D + s0;
    // forward: cumulative true positives
    int carry = 0;
    for (int base = 0; base < nd; base += EV_TILE) {
        const int k0 = base + tid * EV_ITEMS;
        int v[EV_ITEMS], s = 0;
#pragma unroll
        for (int i = 0; i < EV_ITEMS; ++i) { v[i] = k0 + i < nd ? (int)f[k0 + i] : 0; s += v[i]; }
        int excl, total;
        block_scan<int>(s, 0, false, shi, OpAddI(), excl, total);
        int run = carry + excl;
#pragma unroll
        for (int i = 0; i < EV_ITEMS; ++i) {
            run += v[i];
            if (k0 + i < nd) cm[k0 + i] = run;
        }
        carry += total;
    }
    if (npos <= 0) {                               // detections without any ground truth: 0 / 0 on the host
        if (tid == 0) { ap[out] = NAN; rec[out] = NAN; }
        return;
    }
    __syncthreads();                               // cm is read back below by other threads of this workgroup
    // backward: precision envelope (reverse running maximum, 0 behind the end) and the area over the points where recall changes
    const double np_ = (double)npos;
    double env_carry = 0.0, area = 0.0;
    for (int base = (nd - 1) / EV_TILE * EV_TILE; base >= 0; base -= EV_TILE) {
        const int k0 = base + tid * EV_ITEMS;
        int cv[EV_ITEMS + 1];
        cv[0] = (k0 > 0 && k0 - 1 < nd) ? cm[k0 - 1] : 0;
        double p[EV_ITEMS];
#pragma unroll
        for (int i = 0; i < EV_ITEMS; ++i) {
            const bool in = k0 + i < nd;
            cv[i + 1] = in ? cm[k0 + i] : cv[i];
            p[i] = in ? (double)cv[i + 1] / (double)(k0 + i + 1) : 0.0;
        }
        double mine = p[EV_ITEMS - 1];
#pragma unroll
        for (int i = EV_ITEMS - 2; i >= 0; --i) mine = fmax(mine, p[i]);
        double behind, tile_max;
        block_scan<double>(mine, 0.0, true, shd, OpMaxD(), behind, tile_max);
        double env = fmax(behind, env_carry), contrib = 0.0;
#pragma unroll
        for (int i = EV_ITEMS - 1; i >= 0; --i) {
            env = fmax(env, p[i]);
            if (cv[i + 1] != cv[i]) contrib += ((double)cv[i + 1] / np_ - (double)cv[i] / np_) * env;
        }
        double ex_d, tile_sum;
        block_scan<double>(contrib, 0.0, true, shd, OpAddD(), ex_d, tile_sum);
        area += tile_sum;
        env_carry = fmax(env_carry, tile_max);
    }
    if (tid == 0) { ap[out] = (float)area; rec[out] = (float)((double)carry / np_); }
}

static inline int64_t al256(int64_t b) { return (b + 255) & ~(int64_t)255; }
static inline char* align256(void* p) { return (char*)(((uintptr_t)p + 255) & ~(uintptr_t)255); }
static inline int class_bits(int C) { int b = 1; while ((1 << b) <= C) ++b; return b; }      // bits of the values 0 .. C

static int check_sizes(const char* what, int64_t D, int64_t G, int64_t I, int C, int T) {
    if (D < 0 || G < 0 || I < 0 || D >= 0x7f000000LL || G >= 0x7fffffffLL || I >= 0x7fffffffLL || C < 0 || T < 0) {
        set_error("%s: bad sizes (D %lld, G %lld, I %lld, C %d, T %d)", what, (long long)D, (long long)G, (long long)I, C, T);
        return U3D_EINVAL;
    }
    if (C > EV_MAX_C || T > EV_MAX_T) {
        set_error("%s: %d classes / %d thresholds exceed %d / %d", what, C, T, EV_MAX_C, EV_MAX_T);
        return U3D_EUNSUPPORTED;
    }
    return U3D_OK;
}

static int hip_ok(const char* what, hipError_t e) {
    if (e == hipSuccess) return U3D_OK;
    set_error("%s: %s", what, hipGetErrorString(e));
    return U3D_ELAUNCH;
}

}  // namespace u3d

using namespace u3d;

extern "C" {

int u3d_eval_gt_chunk(void) { return EV_GT_CHUNK; }

int64_t u3d_eval_match_ws_bytes(int64_t D, int64_t G) { (void)D; (void)G; return 0; }      // everything goes through LDS

int u3d_eval_match(const float* det_boxes, const int32_t* det_labels, const int32_t* det_off, const float* gt_boxes, const int32_t* gt_labels,
                   const int32_t* gt_off, int64_t D, int64_t G, int64_t I, int C, float* iou_max, int32_t* jmax, int32_t* n_gt, int32_t* n_det,
                   void* ws, u3d_stream_t stream) {
    (void)ws;
    if (int rc = check_sizes("eval_match", D, G, I, C, 0)) return rc;
    if ((D > 0 && (!det_boxes || !det_labels || !iou_max || !jmax)) || (G > 0 && (!gt_boxes || !gt_labels)) ||
        ((D > 0 || G > 0) && (I <= 0 || !det_off || !gt_off)) || (C > 0 && (!n_gt || !n_det))) {
        set_error("eval_match: NULL array for a non-zero size, or rows without images");
        return U3D_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    if (C > 0) {
        if (int rc = hip_ok("eval_match", hipMemsetAsync(n_gt, 0, (size_t)C * 4, s))) return rc;
        if (int rc = hip_ok("eval_match", hipMemsetAsync(n_det, 0, (size_t)C * 4, s))) return rc;
        if (G > 0) hipLaunchKernelGGL(eval_count_k, dim3((unsigned)(ceil_div(G, EV_THREADS) < 256 ? ceil_div(G, EV_THREADS) : 256)), dim3(EV_THREADS), 0, s, gt_labels, G, C, n_gt);
        if (D > 0) hipLaunchKernelGGL(eval_count_k, dim3((unsigned)(ceil_div(D, EV_THREADS) < 256 ? ceil_div(D, EV_THREADS) : 256)), dim3(EV_THREADS), 0, s, det_labels, D, C, n_det);
    }
    if (D > 0)
        hipLaunchKernelGGL(eval_match_k, dim3((unsigned)ceil_div(D, EV_THREADS)), dim3(EV_THREADS), 0, s, det_boxes, det_labels, det_off, gt_boxes,
                           gt_labels, gt_off, (int)D, (int)G, (int)I, C, iou_max, jmax);
    return check_launch("eval_match");
}

int64_t u3d_eval_order_ws_bytes(int64_t D) {
    if (D <= 0 || D >= 0x7fffffffLL) return 0;
    return 2 * al256(D * 8) + u3d_sort_ws_bytes(D, 1) + 512;
}

int u3d_eval_order(const float* det_scores, const int32_t* det_labels, int64_t D, int C, int32_t* perm, void* ws, u3d_stream_t stream) {
    if (int rc = check_sizes("eval_order", D, 0, 0, C, 0)) return rc;
    if (D == 0) return U3D_OK;
    if (!det_scores || !det_labels || !perm || !ws) { set_error("eval_order: NULL array"); return U3D_EINVAL; }
    char* w = align256(ws);
    uint64_t* keys = (uint64_t*)w; w += al256(D * 8);
    uint64_t* sorted = (uint64_t*)w; w += al256(D * 8);
    hipLaunchKernelGGL(eval_keys_k, dim3((unsigned)ceil_div(D, EV_THREADS)), dim3(EV_THREADS), 0, (hipStream_t)stream, det_scores, det_labels, (int)D, C, keys);
    if (int rc = check_launch("eval_order")) return rc;
    return u3d_sort_u64(keys, D, 32 + class_bits(C), sorted, perm, w, stream);
}

int64_t u3d_eval_sweep_ws_bytes(int64_t D, int64_t G, int T) {
    if (D < 0 || G < 0 || T < 0 || T > EV_MAX_T) return 0;
    return al256(T * G * 4) + al256(T * D) + al256(T * D * 4) + 512;
}

int u3d_eval_sweep(const float* iou_max, const int32_t* jmax, const int32_t* perm, const int32_t* n_gt, const int32_t* n_det,
                   const float* thr_host, int64_t D, int64_t G, int C, int T, float* ap, float* rec, uint8_t* tp_flag, int32_t* tp_cum,
                   void* ws, u3d_stream_t stream) {
    if (int rc = check_sizes("eval_sweep", D, G, 0, C, T)) return rc;
    if (C == 0 || T == 0) return U3D_OK;
    if (!n_gt || !n_det || !thr_host || !ap || !rec || (D > 0 && (!iou_max || !jmax || !perm || !ws))) {
        set_error("eval_sweep: NULL array for a non-zero size");
        return U3D_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    EvalThr thr;
    for (int t = 0; t < EV_MAX_T; ++t) thr.v[t] = t < T ? thr_host[t] : INFINITY;
    uint8_t* flag = nullptr;
    int32_t* cum = nullptr;
    if (D > 0) {
        char* w = align256(ws);
        int32_t* claim = (int32_t*)w; w += al256(T * G * 4);
        flag = tp_flag ? tp_flag : (uint8_t*)w; w += al256(T * D);
        cum = tp_cum ? tp_cum : (int32_t*)w;
        const dim3 grid((unsigned)ceil_div(D, EV_THREADS));
        if (G > 0) {
            if (int rc = hip_ok("eval_sweep", hipMemsetAsync(claim, 0x7f, (size_t)T * G * 4, s))) return rc;       // 0x7f7f7f7f: above every rank
            hipLaunchKernelGGL(eval_claim_k, grid, dim3(EV_THREADS), 0, s, iou_max, jmax, perm, (int)D, (int)G, T, thr, claim);
        }
        hipLaunchKernelGGL(eval_flag_k, grid, dim3(EV_THREADS), 0, s, iou_max, jmax, perm, (int)D, (int)G, T, thr, claim, flag);
    }
    hipLaunchKernelGGL(eval_scan_k, dim3((unsigned)C, (unsigned)T), dim3(EV_THREADS), 0, s, flag, n_gt, n_det, (int)D, C, ap, rec, cum);
    return check_launch("eval_sweep");
}

}  // extern "C"
