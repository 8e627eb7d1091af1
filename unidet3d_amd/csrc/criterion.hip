// R12 on the device in five launches (six for a batch with a scene of more than 64 GTs): matcher + classification / box losses
// of all decoder layers and scenes of a batch, forward AND gradients.  The reference: unidet3d/criterion.py:44-178
// UniDet3DCriterion.get_layer_loss / __call__, :200-320 the cost classes and UniMatcher, unidet3d/axis_aligned_iou_loss.py:14-53
// axis_aligned_diou_loss, unidet3d/rotated_iou_loss.py:14-82 diff_diou_rotated_3d / rotated_diou_3d_loss over mmcv's rectangle
// intersection.  Round 3: MIXED batches of the joint config -- every scene carries its own class-column list (dataset), top-k,
// dataset weight and box parametrisation (6-dof axis-aligned or 7-dof with a heading: the rotated DIoU for both the matcher cost
// and the loss, with analytic gradients).
// The torch-op formulation of the same arithmetic costs ~380 launches of [layers, scenes, n, g] tensor ops per step for one
// dataset and a Python loop of ~70 launches per (layer, scene) for a mixed batch; here
//   crit_cost_k   one thread per (layer, query): log-sum-exp of the scene's class columns, cost[q][j] of every GT of the query's
//                 scene (-softmax[label_j] w_cls + box cost w_box, 1e8 where the GT's query mask forbids the query); box cost =
//                 1 - IoU + centre term of GT 0 (the reference's `[:, 0]` quirk of the axis-aligned form) or 1 - rotated DIoU;
//   crit_kth_k    one wave per (layer, scene, GT): the (topk+1)-th smallest cost of the column by k rounds of lexicographic
//                 (value, index) minimum extraction -- the threshold of `cost < values` (:316-319);
//   crit_lse_k + crit_cost_pair_k   the same cost matrix for a batch with a crowded scene (max_gt > 64), where one thread per
//                 query would loop over hundreds of GTs on a grid of a few hundred waves: a pre-pass per (layer, query) stores the
//                 row maximum, the exponential sum and logz, then one thread per (layer, query, GT) entry evaluates the identical
//                 expression (same prob, same box cost, same GT-0 term, same 1e8 sentinel);
//   crit_stats_k  one workgroup per (layer, scene): matched set (W = ceil(max_gt / 64) 64-bit words per query, GT j = bit j & 63
//                 of word j >> 6), class target = label of the LAST matched GT (:98-99 index assignment), weighted cross-entropy
//                 sums and the DIoU sum over matched pairs, reduced in a fixed order (no atomics);
//   crit_final_k  one thread: the scalar loss (means over scenes / scenes with matches, sum over layers) and the per-layer scale
//                 factors of the gradients;
//   crit_grad_k   one thread per (layer, query): d loss / d logits (softmax - one-hot, weighted; zero in the columns of other
//                 datasets) and d loss / d box: the analytic DIoU derivative through _bbox_to_loss for axis-aligned boxes (sub-
//                 gradients of min / max / clamp as torch takes them); for rotated boxes the SAME routine that computes the value
//                 is run on dual numbers (value + 7 tangents), i.e. forward-mode differentiation of exactly the branch taken --
//                 what autograd does to the reference's tensor program.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "u3d_common.h"

namespace u3d {

struct CritParams {
    const float* cls;          // [L][n_tot][CU]
    const float* box;          // [L][n_tot][BD]  (centre, size[, heading]); BD = 6 or 7
    const int32_t* cu;         // [B+1] first query of every scene
    const int32_t* gt_off;     // [B+1] first GT of every scene
    const int64_t* gt_labels;  // [G]   (index into the scene's class list)
    const float* gt_boxes;     // [G][BD]
    const uint8_t* qmask;      // scene b: [g_b][n_b] at qm_off[b]
    const int64_t* qm_off;     // [B+1]; also the offset of scene b's [n_b][g_b] block in `cost`
    const int32_t* meta;       // [B][4]: classes + 1 of the scene's dataset, top-k, 1 = boxes carry a heading, offset into cidx
    const float* scene_w;      // [B] dataset weight
    const int32_t* cidx;       // class columns of every scene in the CU-wide logit rows (concatenated); nullptr = columns 0..C1-1
    int L, B, CU, BD;
    int W;                     // 64-bit words of a query's matched-GT set: ceil(max_gt / 64), at least 1
    int64_t n_tot, G, P;       // P = sum n_b g_b
    float w_cls, w_box, non_obj_w, lw_cls, lw_box;
    // workspace
    float* cost;               // [L][P]
    float* logz;               // [L][n_tot]
    float* kth;                // [L][G]
    unsigned long long* mm;    // [L][n_tot][W] matched-GT bit mask
    float* stats;              // [L][B][4]: sum w, sum w nll, matched pairs, sum diou
    float* scale;              // [L][2]: (unused, number of scenes with matches) -- written by crit_final_k
    float* mxse;               // [L][n_tot][2]: (row maximum, exponential sum) of crit_lse_k; only with max_gt > 64
    float* loss;               // [1]
    float* dcls;
    float* dbox;
};

__device__ __forceinline__ int scene_of(const int32_t* cu, int B, int q) {
    int lo = 0, hi = B;                    // cu[lo] <= q < cu[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (cu[mid] <= q) lo = mid; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ int col_of(const CritParams& p, int b, int c) { return p.cidx ? p.cidx[p.meta[b * 4 + 3] + c] : c; }

struct Box6 { float p1[3], p2[3]; };
__device__ __forceinline__ Box6 corners(const float* b) {      // _bbox_to_loss (criterion.py:180-198)
    Box6 r;
#pragma unroll
    for (int a = 0; a < 3; ++a) { r.p1[a] = b[a] - b[3 + a] / 2; r.p2[a] = b[a] + b[3 + a] / 2; }
    return r;
}
__device__ __forceinline__ float iou3(const Box6& p, const Box6& t) {      // mmdet3d AxisAlignedBboxOverlaps3D(is_aligned=True), eps 1e-6
    float inter = 1.f, vp = 1.f, vt = 1.f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        inter *= fmaxf(fminf(p.p2[a], t.p2[a]) - fmaxf(p.p1[a], t.p1[a]), 0.f);
        vp *= p.p2[a] - p.p1[a];
        vt *= t.p2[a] - t.p1[a];
    }
    return inter / fmaxf(vp + vt - inter, 1e-6f);
}
__device__ __forceinline__ float centre_term(const Box6& p, const Box6& t) {     // r2 / c2 (axis_aligned_iou_loss.py:30-49)
    float r2 = 0.f, c2 = 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float d = (p.p1[a] + p.p2[a]) / 2 - (t.p1[a] + t.p2[a]) / 2;
        const float e = fminf(p.p1[a], t.p1[a]) - fmaxf(p.p2[a], t.p2[a]);
        r2 += d * d;
        c2 += e * e;
    }
    return r2 / c2;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Rotated DIoU (unidet3d/rotated_iou_loss.py:14-60 over mmcv.ops.diff_iou_rotated: box2corners, box_intersection,
// box1_in_box2, build_vertices, sort_indices, calculate_area), one (prediction, target) pair, on a scalar type S that is either
// float (values: the matcher's cost matrix) or Dual (value + tangents w.r.t. the 7 parameters of the predicted box: the loss
// gradient).  Same stages and constants as the tensor-op formulation in unidet3d_amd/criterion.py, which is pinned by the
// reference's golden vectors (tests/golden/ref_criterion.npz F.rot, C2): corners, 16 edge-edge intersections with the strict
// 0 < t, u < 1 test (point = a + t2 (b - a), t2 = den_t / (num + 1e-8)), corners of one rectangle inside the other (1e-6 slack),
// repeated candidates dropped (the first copy stays), the rest ordered by angle around their mean (no gradient through the order),
// shoelace area, |.|, zero below 3 vertices.
struct Dual {
    float v, d[7];
    __device__ __forceinline__ Dual() {}
    __device__ __forceinline__ Dual(float x) : v(x) {
#pragma unroll
        for (int i = 0; i < 7; ++i) d[i] = 0.f;
    }
};
__device__ __forceinline__ Dual dual_var(float x, int i) { Dual r(x); r.d[i] = 1.f; return r; }
__device__ __forceinline__ float val(float x) { return x; }
__device__ __forceinline__ float val(const Dual& x) { return x.v; }
__device__ __forceinline__ Dual operator+(const Dual& a, const Dual& b) { Dual r; r.v = a.v + b.v;
#pragma unroll
    for (int i = 0; i < 7; ++i) r.d[i] = a.d[i] + b.d[i]; return r; }
__device__ __forceinline__ Dual operator-(const Dual& a, const Dual& b) { Dual r; r.v = a.v - b.v;
#pragma unroll
    for (int i = 0; i < 7; ++i) r.d[i] = a.d[i] - b.d[i]; return r; }
__device__ __forceinline__ Dual operator-(const Dual& a) { Dual r; r.v = -a.v;
#pragma unroll
    for (int i = 0; i < 7; ++i) r.d[i] = -a.d[i]; return r; }
__device__ __forceinline__ Dual operator*(const Dual& a, const Dual& b) { Dual r; r.v = a.v * b.v;
#pragma unroll
    for (int i = 0; i < 7; ++i) r.d[i] = a.d[i] * b.v + a.v * b.d[i]; return r; }
__device__ __forceinline__ Dual operator/(const Dual& a, const Dual& b) { Dual r; const float inv = 1.f / b.v; r.v = a.v * inv;
#pragma unroll
    for (int i = 0; i < 7; ++i) r.d[i] = (a.d[i] - r.v * b.d[i]) * inv; return r; }
__device__ __forceinline__ Dual operator*(float a, const Dual& b) { Dual r; r.v = a * b.v;
#pragma unroll
    for (int i = 0; i < 7; ++i) r.d[i] = a * b.d[i]; return r; }
__device__ __forceinline__ Dual operator+(const Dual& a, float b) { Dual r = a; r.v += b; return r; }
__device__ __forceinline__ Dual scaled(const Dual& a, float k) { return k * a; }
__device__ __forceinline__ float scaled(float a, float k) { return k * a; }
__device__ __forceinline__ void sincos_of(float a, float& s, float& c) { s = sinf(a); c = cosf(a); }
__device__ __forceinline__ void sincos_of(const Dual& a, Dual& s, Dual& c) {
    const float sv = sinf(a.v), cv = cosf(a.v);
    s.v = sv; c.v = cv;
#pragma unroll
    for (int i = 0; i < 7; ++i) { s.d[i] = cv * a.d[i]; c.d[i] = -sv * a.d[i]; }
}
// torch.maximum / torch.minimum: the gradient of a tie is split evenly; clamp(min=0) passes the gradient for x >= 0; |x| has sign(x)
template <typename S> __device__ __forceinline__ S max2(const S& a, const S& b) { return val(a) > val(b) ? a : (val(a) < val(b) ? b : scaled(a + b, 0.5f)); }
template <typename S> __device__ __forceinline__ S min2(const S& a, const S& b) { return val(a) < val(b) ? a : (val(a) > val(b) ? b : scaled(a + b, 0.5f)); }
template <typename S> __device__ __forceinline__ S relu0(const S& a) { return val(a) >= 0.f ? a : S(0.f); }
template <typename S> __device__ __forceinline__ S abs_of(const S& a) { return val(a) > 0.f ? a : (val(a) < 0.f ? S(0.f) - a : S(0.f)); }
// x.max(-1)[0] / x.min(-1)[0] over the 4 corners: the gradient goes to the FIRST extremal entry
template <typename S> __device__ __forceinline__ S max4(const S (&x)[4]) { int k = 0;
#pragma unroll
    for (int i = 1; i < 4; ++i) if (val(x[i]) > val(x[k])) k = i; return x[k]; }
template <typename S> __device__ __forceinline__ S min4(const S (&x)[4]) { int k = 0;
#pragma unroll
    for (int i = 1; i < 4; ++i) if (val(x[i]) < val(x[k])) k = i; return x[k]; }

template <typename S>
__device__ __forceinline__ void box2corners(const S& x, const S& y, const S& w, const S& h, const S& a, S (&cx)[4], S (&cy)[4]) {
    S s, c;
    sincos_of(a, s, c);
    const float sx[4] = {0.5f, -0.5f, -0.5f, 0.5f}, sy[4] = {0.5f, 0.5f, -0.5f, -0.5f};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const S x4 = scaled(w, sx[i]), y4 = scaled(h, sy[i]);
        cx[i] = x4 * c - y4 * s + x;
        cy[i] = x4 * s + y4 * c + y;
    }
}

// corners of rectangle 1 inside rectangle 2 (mmcv box1_in_box2): values only
template <typename S>
__device__ __forceinline__ void corners_inside(const S (&x1)[4], const S (&y1)[4], const S (&x2)[4], const S (&y2)[4], bool (&in)[4]) {
    const float ax = val(x2[0]), ay = val(y2[0]);
    const float abx = val(x2[1]) - ax, aby = val(y2[1]) - ay, adx = val(x2[3]) - ax, ady = val(y2[3]) - ay;
    const float nab = abx * abx + aby * aby, nad = adx * adx + ady * ady;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float amx = val(x1[i]) - ax, amy = val(y1[i]) - ay;
        const float pab = (abx * amx + aby * amy) / nab, pad = (adx * amx + ady * amy) / nad;
        in[i] = pab > -1e-6f && pab < 1.f + 1e-6f && pad > -1e-6f && pad < 1.f + 1e-6f;
    }
}

// A candidate that repeats an earlier one (coincident boxes: every corner of one is a corner of the other) is passed over, as mmcv's
// vertex sort does (it only moves on to a vertex strictly after the previous one): the FIRST copy stays, so the predicted box's own
// corner carries the gradient.  Left in, the copies share an angle and the polygon's visiting order -- and with it the gradient --
// would depend on the order of equal keys.  Values only; kept out of line so that the callers' code does not grow with it.
__device__ __noinline__ void drop_repeated_values(const float* x, const float* y, bool* ok) {
    for (int k = 1; k < 24; ++k) {
        if (!ok[k]) continue;
        for (int j = 0; j < k; ++j)
            if (ok[j] && fabsf(x[k] - x[j]) <= 1e-8f && fabsf(y[k] - y[j]) <= 1e-8f) { ok[k] = false; break; }
    }
}
template <typename S> __device__ __forceinline__ void drop_repeated(const S (&vx)[24], const S (&vy)[24], bool (&ok)[24]) {
    float x[24], y[24];
#pragma unroll
    for (int k = 0; k < 24; ++k) { x[k] = val(vx[k]); y[k] = val(vy[k]); }
    drop_repeated_values(x, y, ok);
}

// 1 - DIoU of a predicted box p and a target t, both (x, y, z, w, h, l, alpha)
template <typename S>
__device__ S rotated_diou_loss(const S (&p)[7], const float (&tf)[7]) {
    S t[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) t[i] = S(tf[i]);
    S x1[4], y1[4], x2[4], y2[4];
    box2corners(p[0], p[1], p[3], p[4], p[6], x1, y1);
    box2corners(t[0], t[1], t[3], t[4], t[6], x2, y2);
    // ---- candidate vertices: 4 + 4 corners, 16 edge intersections ----
    S vx[24], vy[24];
    bool ok[24];
    {
        bool in1[4], in2[4];
        corners_inside(x1, y1, x2, y2, in1);
        corners_inside(x2, y2, x1, y1, in2);
#pragma unroll
        for (int i = 0; i < 4; ++i) { vx[i] = x1[i]; vy[i] = y1[i]; ok[i] = in1[i]; vx[4 + i] = x2[i]; vy[4 + i] = y2[i]; ok[4 + i] = in2[i]; }
    }
    for (int i = 0; i < 4; ++i) {
        const S &ax = x1[i], &ay = y1[i], &bx = x1[(i + 1) & 3], &by = y1[(i + 1) & 3];
        for (int j = 0; j < 4; ++j) {
            const S &cx = x2[j], &cy = y2[j], &dx = x2[(j + 1) & 3], &dy = y2[(j + 1) & 3];
            const S num = (ax - bx) * (cy - dy) - (ay - by) * (cx - dx);
            const S den_t = (ax - cx) * (cy - dy) - (ay - cy) * (cx - dx);
            const S den_u = (ax - bx) * (ay - cy) - (ay - by) * (ax - cx);
            const float nv = val(num);
            bool m = false;
            if (nv != 0.f) {
                const float tt = val(den_t) / nv, uu = -val(den_u) / nv;
                m = tt > 0.f && tt < 1.f && uu > 0.f && uu < 1.f;
            }
            const int k = 8 + i * 4 + j;
            ok[k] = m;
            if (m) {
                const S t2 = den_t / (num + 1e-8f);
                vx[k] = ax + t2 * (bx - ax);
                vy[k] = ay + t2 * (by - ay);
            } else {
                vx[k] = S(0.f); vy[k] = S(0.f);
            }
        }
    }
    drop_repeated(vx, vy, ok);
    // ---- order the valid candidates by angle around their mean (values only), shoelace area ----
    int nvert = 0;
    float mx = 0.f, my = 0.f;
    for (int k = 0; k < 24; ++k)
        if (ok[k]) { ++nvert; mx += val(vx[k]); my += val(vy[k]); }
    S inter(0.f);
    if (nvert >= 3) {
        mx /= nvert; my /= nvert;
        int ord[24];
        float ang[24];
        int n = 0;
        for (int k = 0; k < 24; ++k)
            if (ok[k]) {                      // stable insertion by (angle, index)
                const float a = atan2f(val(vy[k]) - my, val(vx[k]) - mx);
                int pos = n;
                while (pos > 0 && ang[pos - 1] > a) { ang[pos] = ang[pos - 1]; ord[pos] = ord[pos - 1]; --pos; }
                ang[pos] = a; ord[pos] = k; ++n;
            }
        S area(0.f);
        for (int a = 0; a < n; ++a) {
            const int k0 = ord[a], k1 = ord[a + 1 == n ? 0 : a + 1];
            area = area + (vx[k0] * vy[k1] - vy[k0] * vx[k1]);
        }
        inter = scaled(abs_of(area), 0.5f);
    }
    // ---- third dimension, union, enclosing box, centre term (rotated_iou_loss.py:27-60) ----
    const S zmax1 = p[2] + scaled(p[5], 0.5f), zmin1 = p[2] - scaled(p[5], 0.5f);
    const S zmax2 = t[2] + scaled(t[5], 0.5f), zmin2 = t[2] - scaled(t[5], 0.5f);
    const S inter3 = inter * relu0(min2(zmax1, zmax2) - max2(zmin1, zmin2));
    const S uni = p[3] * p[4] * p[5] + t[3] * t[4] * t[5] - inter3;
    const S ex = min2(min4(x1), min4(x2)) - max2(max4(x1), max4(x2));
    const S ey = min2(min4(y1), min4(y2)) - max2(max4(y1), max4(y2));
    const S ez = min2(zmin1, zmin2) - max2(zmax1, zmax2);
    // the reference's centre term runs over the first three entries of the BEV vectors (x, y, w) -- not (x, y, z) (:58)
    const S d0 = p[0] - t[0], d1 = p[1] - t[1], d2 = p[3] - t[3];
    const S r2 = d0 * d0 + d1 * d1 + d2 * d2;
    const S c2 = ex * ex + ey * ey + ez * ez;
    return S(1.f) - (inter3 / uni - r2 / c2);
}

__device__ __forceinline__ float rot_cost(const float* pb, const float* gb) {
    float p[7], t[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) { p[i] = pb[i]; t[i] = gb[i]; }
    return rotated_diou_loss<float>(p, t);
}

__global__ __launch_bounds__(256) void crit_cost_k(CritParams p) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)p.L * p.n_tot) return;
    const int l = (int)(idx / p.n_tot), q = (int)(idx % p.n_tot);
    const int b = scene_of(p.cu, p.B, q);
    const int C1 = p.meta[b * 4], yaw = p.meta[b * 4 + 2];
    const float* x = p.cls + idx * p.CU;
    float mx = -INFINITY;
    for (int c = 0; c < C1; ++c) mx = fmaxf(mx, x[col_of(p, b, c)]);
    float se = 0.f;
    for (int c = 0; c < C1; ++c) se += expf(x[col_of(p, b, c)] - mx);
    p.logz[idx] = mx + logf(se);
    const int g0 = p.gt_off[b], g = p.gt_off[b + 1] - g0;
    if (g == 0) return;
    const int ql = q - p.cu[b], n = p.cu[b + 1] - p.cu[b];
    const float* pbox = p.box + idx * p.BD;
    const Box6 pb = corners(pbox);
    const float rc0 = yaw ? 0.f : centre_term(pb, corners(p.gt_boxes + (int64_t)g0 * p.BD));       // the `[:, 0]` term: GT 0 of the scene for every GT
    float* crow = p.cost + (int64_t)l * p.P + p.qm_off[b] + (int64_t)ql * g;
    const uint8_t* qm = p.qmask + p.qm_off[b];
    for (int j = 0; j < g; ++j) {
        float c = 1e8f;
        if (qm[(int64_t)j * n + ql]) {
            const float prob = expf(x[col_of(p, b, (int)p.gt_labels[g0 + j])] - mx) / se;
            const float* gb = p.gt_boxes + (int64_t)(g0 + j) * p.BD;
            const float box_cost = yaw ? rot_cost(pbox, gb) : (1.f - iou3(pb, corners(gb))) + rc0;
            c = -prob * p.w_cls + box_cost * p.w_box;
        }
        crow[j] = c;
    }
}

// ---- the cost matrix of a batch with a crowded scene (max_gt > 64): the log-sum-exp pre-pass, then one thread per entry ----
__global__ __launch_bounds__(256) void crit_lse_k(CritParams p) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)p.L * p.n_tot) return;
    const int q = (int)(idx % p.n_tot);
    const int b = scene_of(p.cu, p.B, q);
    const int C1 = p.meta[b * 4];
    const float* x = p.cls + idx * p.CU;
    float mx = -INFINITY;
    for (int c = 0; c < C1; ++c) mx = fmaxf(mx, x[col_of(p, b, c)]);
    float se = 0.f;
    for (int c = 0; c < C1; ++c) se += expf(x[col_of(p, b, c)] - mx);
    p.logz[idx] = mx + logf(se);
    p.mxse[idx * 2] = mx;
    p.mxse[idx * 2 + 1] = se;
}

// One thread per (layer, query, GT) entry of `cost`, entries in storage order ([L][P]; scene b's [n_b][g_b] block at qm_off[b]), so
// the 64 lanes of a wave hold consecutive GTs of one query (or of neighbouring queries): coalesced stores and GT box loads, the query's
// own row is a broadcast.  Blocks of one wave: a rotated pair is a long, divergent, register-heavy evaluation with no cooperation
// between threads, so the wave is the natural scheduling unit and a crowded scene's few thousand waves spread over every CU.
__global__ __launch_bounds__(64) void crit_cost_pair_k(CritParams p) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= p.P) return;
    const int l = blockIdx.y;
    int b = 0;
    {
        int hi = p.B;                          // qm_off[b] <= e < qm_off[hi]; scenes without GT are empty ranges and are passed over
        while (hi - b > 1) {
            const int mid = (b + hi) >> 1;
            if (p.qm_off[mid] <= e) b = mid; else hi = mid;
        }
    }
    const int g0 = p.gt_off[b], g = p.gt_off[b + 1] - g0;
    const int n = p.cu[b + 1] - p.cu[b];
    const int64_t r = e - p.qm_off[b];
    if (g <= 0 || r >= (int64_t)n * g) return;       // P and qm_off disagree: nothing to index
    const int ql = (int)(r / g), j = (int)(r % g);
    float c = 1e8f;
    if (p.qmask[p.qm_off[b] + (int64_t)j * n + ql]) {
        const int yaw = p.meta[b * 4 + 2];
        const int64_t idx = (int64_t)l * p.n_tot + p.cu[b] + ql;
        const float* x = p.cls + idx * p.CU;
        const float mx = p.mxse[idx * 2], se = p.mxse[idx * 2 + 1];
        const float* pbox = p.box + idx * p.BD;
        const Box6 pb = corners(pbox);
        const float rc0 = yaw ? 0.f : centre_term(pb, corners(p.gt_boxes + (int64_t)g0 * p.BD));       // the `[:, 0]` term, as in crit_cost_k
        const float prob = expf(x[col_of(p, b, (int)p.gt_labels[g0 + j])] - mx) / se;
        const float* gb = p.gt_boxes + (int64_t)(g0 + j) * p.BD;
        const float box_cost = yaw ? rot_cost(pbox, gb) : (1.f - iou3(pb, corners(gb))) + rc0;
        c = -prob * p.w_cls + box_cost * p.w_box;
    }
    p.cost[(int64_t)l * p.P + e] = c;
}

// one wave per (layer, GT): kth = (topk+1)-th smallest cost of the GT's column
__global__ __launch_bounds__(64) void crit_kth_k(CritParams p) {
    const int64_t wid = blockIdx.x;
    if (wid >= (int64_t)p.L * p.G) return;
    const int l = (int)(wid / p.G), gj = (int)(wid % p.G);
    int b = 0;
    while (b + 1 < p.B && p.gt_off[b + 1] <= gj) ++b;
    const int g0 = p.gt_off[b], g = p.gt_off[b + 1] - g0, j = gj - g0;
    const int n = p.cu[b + 1] - p.cu[b];
    const int topk = p.meta[b * 4 + 1];
    const float* col = p.cost + (int64_t)l * p.P + p.qm_off[b] + j;
    const int lane = threadIdx.x;
    float pv = -INFINITY;
    int pi = -1;
    for (int r = 0; r <= topk; ++r) {              // r-th smallest in (value, index) order, duplicates counted
        float bv = INFINITY;
        int bi = 0x7fffffff;
        for (int q = lane; q < n; q += 64) {
            const float v = col[(int64_t)q * g];
            const bool after = v > pv || (v == pv && q > pi);
            if (after && (v < bv || (v == bv && q < bi))) { bv = v; bi = q; }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ov < bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        pv = bv; pi = bi;
    }
    if (lane == 0) p.kth[(int64_t)l * p.G + gj] = pv;
}

__global__ __launch_bounds__(256) void crit_stats_k(CritParams p) {
    const int l = blockIdx.x / p.B, b = blockIdx.x % p.B;
    const int q0 = p.cu[b], n = p.cu[b + 1] - q0;
    const int g0 = p.gt_off[b], g = p.gt_off[b + 1] - g0;
    const int n_cls = p.meta[b * 4] - 1, yaw = p.meta[b * 4 + 2];
    float sw = 0.f, swn = 0.f, cnt = 0.f, sd = 0.f;
    for (int ql = threadIdx.x; ql < n; ql += 256) {
        const int64_t idx = (int64_t)l * p.n_tot + q0 + ql;
        int last = -1;
        const float* crow = p.cost + (int64_t)l * p.P + p.qm_off[b] + (int64_t)ql * g;
        const float* kth = p.kth + (int64_t)l * p.G + g0;
        const float* pbox = p.box + idx * p.BD;
        const Box6 pb = corners(pbox);
        for (int w = 0; w < p.W; ++w) {              // GTs in ascending order, 64 to a word; a word past the scene's GTs is written as 0
            unsigned long long m = 0ull;
            const int j1 = min(g, (w + 1) * 64);
            for (int j = w * 64; j < j1; ++j)
                if (crow[j] < kth[j]) {
                    m |= 1ull << (j & 63);
                    last = j;
                    const float* gb = p.gt_boxes + (int64_t)(g0 + j) * p.BD;
                    if (yaw) {
                        sd += rot_cost(pbox, gb);
                    } else {
                        const Box6 tb = corners(gb);
                        sd += (1.f - iou3(pb, tb)) + centre_term(pb, tb);
                    }
                    cnt += 1.f;
                }
            p.mm[idx * p.W + w] = m;
        }
        const int target = last >= 0 ? (int)p.gt_labels[g0 + last] : n_cls;
        const float w = target == n_cls ? p.non_obj_w : 1.f;
        sw += w;
        swn += w * (p.logz[idx] - p.cls[idx * p.CU + col_of(p, b, target)]);
    }
    // fixed-order block reduction
    __shared__ float red[4][256];
    red[0][threadIdx.x] = sw; red[1][threadIdx.x] = swn; red[2][threadIdx.x] = cnt; red[3][threadIdx.x] = sd;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (threadIdx.x < s)
#pragma unroll
            for (int k = 0; k < 4; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x < 4) p.stats[((int64_t)l * p.B + b) * 4 + threadIdx.x] = red[threadIdx.x][0];
}

__global__ void crit_final_k(CritParams p) {
    if (threadIdx.x || blockIdx.x) return;
    float total = 0.f;
    for (int l = 0; l < p.L; ++l) {
        float cls_sum = 0.f, box_sum = 0.f, n_has = 0.f;
        for (int b = 0; b < p.B; ++b) {
            const float* s = p.stats + ((int64_t)l * p.B + b) * 4;
            cls_sum += p.scene_w[b] * (s[1] / s[0]);
            if (s[2] > 0.f) { box_sum += p.scene_w[b] * (s[3] / s[2]); n_has += 1.f; }
        }
        total += p.lw_cls * (cls_sum / p.B) + p.lw_box * (box_sum / fmaxf(n_has, 1.f));
        p.scale[l * 2 + 1] = n_has;
    }
    p.loss[0] = total;
}

__device__ __forceinline__ float pick_gt(float a, float b) { return a > b ? 1.f : (a == b ? 0.5f : 0.f); }     // d max(a, b) / d a
__device__ __forceinline__ float pick_lt(float a, float b) { return a < b ? 1.f : (a == b ? 0.5f : 0.f); }     // d min(a, b) / d a

// MULTI = false: one mask word per query (max_gt <= 64) -- the statements of the kernel as it was before the multi-word masks, so
// that the compiler sees the same program and loss / dcls / dbox of such batches keep their bits (the rotated branch is sensitive
// to how the surrounding code is shaped: DESIGN.md 4.8).  MULTI = true: W words, scanned from the top for the last matched GT and
// walked in ascending order for the box gradient.
template <bool MULTI>
__global__ __launch_bounds__(256) void crit_grad_k(CritParams p) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)p.L * p.n_tot) return;
    const int l = (int)(idx / p.n_tot), q = (int)(idx % p.n_tot);
    const int b = scene_of(p.cu, p.B, q);
    const int g0 = p.gt_off[b];
    const int C1 = p.meta[b * 4], n_cls = C1 - 1, yaw = p.meta[b * 4 + 2];
    const float ds_w = p.scene_w[b];
    const float* st = p.stats + ((int64_t)l * p.B + b) * 4;
    const unsigned long long* mq = p.mm + idx * (MULTI ? p.W : 1);
    const unsigned long long m = MULTI ? 0ull : mq[0];
    // ---- classification: lw_cls * ds_w / B * w_q / sum_w * (softmax - onehot(target)); zero in the other datasets' columns ----
    int last = m ? 63 - __clzll(m) : -1;
    if constexpr (MULTI) {                          // the highest matched GT: the words from the top
        for (int w = p.W - 1; w >= 0; --w) {
            const unsigned long long mw = mq[w];
            if (mw) { last = w * 64 + 63 - __clzll(mw); break; }
        }
    }
    const bool any = MULTI ? last >= 0 : m != 0ull;
    const int target = last >= 0 ? (int)p.gt_labels[g0 + last] : n_cls;
    const float w = target == n_cls ? p.non_obj_w : 1.f;
    const float kc = p.lw_cls * ds_w / p.B * w / st[0];
    const float* x = p.cls + idx * p.CU;
    float* dx = p.dcls + idx * p.CU;
    const float lz = p.logz[idx];
    if (p.cidx)
        for (int c = 0; c < p.CU; ++c) dx[c] = 0.f;
    for (int c = 0; c < C1; ++c) {
        const int col = col_of(p, b, c);
        dx[col] = kc * (expf(x[col] - lz) - (c == target ? 1.f : 0.f));
    }
    // ---- boxes: lw_box * ds_w / (n_has * cnt) * sum over matched GTs of d diou / d box ----
    float* db = p.dbox + idx * p.BD;
    if (yaw) {
        float gacc[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (any) {
            const float kb = p.lw_box * ds_w / (fmaxf(p.scale[l * 2 + 1], 1.f) * st[2]);
            Dual pd[7];
#pragma unroll
            for (int i = 0; i < 7; ++i) pd[i] = dual_var(p.box[idx * 7 + i], i);
            auto add_gt = [&](int j) {
                float t[7];
#pragma unroll
                for (int i = 0; i < 7; ++i) t[i] = p.gt_boxes[(int64_t)(g0 + j) * 7 + i];
                const Dual r = rotated_diou_loss<Dual>(pd, t);
#pragma unroll
                for (int i = 0; i < 7; ++i) gacc[i] += r.d[i];
            };
            if constexpr (MULTI) {                   // ascending GT order: words in ascending order, bits from the lowest
                for (int w = 0; w < p.W; ++w)
                    for (unsigned long long mmask = mq[w]; mmask; mmask &= mmask - 1) add_gt(w * 64 + __ffsll((long long)mmask) - 1);
            } else {
                for (unsigned long long mmask = m; mmask; mmask &= mmask - 1) add_gt(__ffsll((long long)mmask) - 1);
            }
#pragma unroll
            for (int i = 0; i < 7; ++i) gacc[i] *= kb;
        }
#pragma unroll
        for (int i = 0; i < 7; ++i) db[i] = gacc[i];
        return;
    }
    float gc[3] = {0.f, 0.f, 0.f}, gs[3] = {0.f, 0.f, 0.f};
    if (any) {
        const float kb = p.lw_box * ds_w / (fmaxf(p.scale[l * 2 + 1], 1.f) * st[2]);
        const Box6 pb = corners(p.box + idx * p.BD);
        for (int w = 0; w < (MULTI ? p.W : 1); ++w)
        for (unsigned long long mmask = MULTI ? mq[w] : m; mmask; mmask &= mmask - 1) {
            const int j = (MULTI ? w * 64 : 0) + __ffsll((long long)mmask) - 1;
            const Box6 tb = corners(p.gt_boxes + (int64_t)(g0 + j) * p.BD);
            float wh[3], dd[3], lo[3], hi[3];
            float inter = 1.f, vp = 1.f, vt = 1.f, r2 = 0.f, c2 = 0.f;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                lo[a] = fmaxf(pb.p1[a], tb.p1[a]); hi[a] = fminf(pb.p2[a], tb.p2[a]);
                wh[a] = fmaxf(hi[a] - lo[a], 0.f);
                dd[a] = pb.p2[a] - pb.p1[a];
                inter *= wh[a]; vp *= dd[a]; vt *= tb.p2[a] - tb.p1[a];
                const float d = (pb.p1[a] + pb.p2[a]) / 2 - (tb.p1[a] + tb.p2[a]) / 2;
                const float e = fminf(pb.p1[a], tb.p1[a]) - fmaxf(pb.p2[a], tb.p2[a]);
                r2 += d * d; c2 += e * e;
            }
            const float un_raw = vp + vt - inter;
            const float un = fmaxf(un_raw, 1e-6f);
            const float un_live = pick_gt(un_raw, 1e-6f);          // union = max(., eps): gradient reaches the volumes only when not clamped
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const int a1 = (a + 1) % 3, a2 = (a + 2) % 3;
                const float clamp_live = (hi[a] - lo[a]) >= 0.f ? 1.f : 0.f;            // clamp(min=0) passes the gradient for x >= 0
                const float di_lo = -wh[a1] * wh[a2] * clamp_live, di_hi = wh[a1] * wh[a2] * clamp_live;     // d inter / d lo_a, d hi_a
                const float di1 = di_lo * pick_gt(pb.p1[a], tb.p1[a]), di2 = di_hi * pick_lt(pb.p2[a], tb.p2[a]);
                const float dv1 = -dd[a1] * dd[a2], dv2 = dd[a1] * dd[a2];
                const float du1 = un_live * (dv1 - di1), du2 = un_live * (dv2 - di2);
                const float diou1 = (di1 * un - inter * du1) / (un * un), diou2 = (di2 * un - inter * du2) / (un * un);
                const float d = (pb.p1[a] + pb.p2[a]) / 2 - (tb.p1[a] + tb.p2[a]) / 2;
                const float e = fminf(pb.p1[a], tb.p1[a]) - fmaxf(pb.p2[a], tb.p2[a]);
                const float dr = d;                                                            // d r2 / d p1_a = d r2 / d p2_a
                const float dc1 = 2.f * e * pick_lt(pb.p1[a], tb.p1[a]), dc2 = -2.f * e * pick_gt(pb.p2[a], tb.p2[a]);
                const float g1 = -diou1 + (dr * c2 - r2 * dc1) / (c2 * c2);
                const float g2 = -diou2 + (dr * c2 - r2 * dc2) / (c2 * c2);
                gc[a] += g1 + g2;                      // p1 = c - s/2, p2 = c + s/2
                gs[a] += (g2 - g1) / 2;
            }
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) { gc[a] *= kb; gs[a] *= kb; }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) { db[a] = gc[a]; db[3 + a] = gs[a]; }
    if (p.BD == 7) db[6] = 0.f;                        // a yaw-free scene of a mixed batch: the heading column is not used
}

// ---- box decode of a yaw-free head: PredBBox's exp + _bbox_pred_to_bbox (unidet3d/encoder.py:99-111, :241-271) in one pass ----
// raw [M][8] (Linear output; the two angle columns are unused here), centres [M][3] -> box [M][6]:
//   e_i = exp(raw_i), i < 6;  centre_a = c_a + (e_{2a+1} - e_{2a}) / 2;  size_a = e_{2a} + e_{2a+1}
__global__ __launch_bounds__(256) void box_decode_fwd_k(const float* __restrict__ raw, const float* __restrict__ cen, int64_t M, float* __restrict__ box) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    const float4 r0 = reinterpret_cast<const float4*>(raw + i * 8)[0], r1 = reinterpret_cast<const float4*>(raw + i * 8)[1];
    const float e[6] = {expf(r0.x), expf(r0.y), expf(r0.z), expf(r0.w), expf(r1.x), expf(r1.y)};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        box[i * 6 + a] = cen[i * 3 + a] + (e[2 * a + 1] - e[2 * a]) / 2;
        box[i * 6 + 3 + a] = e[2 * a] + e[2 * a + 1];
    }
}
__global__ __launch_bounds__(256) void box_decode_bwd_k(const float* __restrict__ raw, const float* __restrict__ dbox, int64_t M, float* __restrict__ draw) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    const float4 r0 = reinterpret_cast<const float4*>(raw + i * 8)[0], r1 = reinterpret_cast<const float4*>(raw + i * 8)[1];
    const float e[6] = {expf(r0.x), expf(r0.y), expf(r0.z), expf(r0.w), expf(r1.x), expf(r1.y)};
    float g[8];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float dc = dbox[i * 6 + a], ds = dbox[i * 6 + 3 + a];
        g[2 * a] = e[2 * a] * (ds - dc / 2);
        g[2 * a + 1] = e[2 * a + 1] * (ds + dc / 2);
    }
    g[6] = 0.f; g[7] = 0.f;
    reinterpret_cast<float4*>(draw + i * 8)[0] = make_float4(g[0], g[1], g[2], g[3]);
    reinterpret_cast<float4*>(draw + i * 8)[1] = make_float4(g[4], g[5], g[6], g[7]);
}

// ---- box decode of a head WITH a heading (7-dof), or of a mixed batch: PredBBox's exp + _bbox_pred_to_bbox incl. its rotated branch
// (unidet3d/encoder.py:99-111, :241-283) in one pass each way.  raw [M][8], centres [M][3], yaw [M] bytes (nullable = every row has a
// heading) -> box [M][7]:
//   rows with a heading:  (centre, w = S / (1 + q), l = w q, size_z, alpha)   S = e0 + e1 + e2 + e3, q = exp(sqrt(r6^2 + r7^2)),
//                                                                            alpha = atan2(r6, r7) / 2
//   rows without (scenes of the yaw-free datasets of a mixed batch, whose heading columns the reference never evaluates,
//   encoder.py:186-199):  (centre, size_x, size_y, size_z, 0); their raw heading columns receive a zero gradient.
// Replaces ~25 element-wise launches forward and ~50 backward per decoder head of the joint config (7 heads per step).
__global__ __launch_bounds__(256) void box_decode7_fwd_k(const float* __restrict__ raw, const float* __restrict__ cen, const uint8_t* __restrict__ yaw,
                                                         int64_t M, float* __restrict__ box) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    const float4 r0 = reinterpret_cast<const float4*>(raw + i * 8)[0], r1 = reinterpret_cast<const float4*>(raw + i * 8)[1];
    const float e[6] = {expf(r0.x), expf(r0.y), expf(r0.z), expf(r0.w), expf(r1.x), expf(r1.y)};
    float o[7];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        o[a] = cen[i * 3 + a] + (e[2 * a + 1] - e[2 * a]) / 2;
        o[3 + a] = e[2 * a] + e[2 * a + 1];
    }
    o[6] = 0.f;
    if (!yaw || yaw[i]) {
        const float S = e[0] + e[1] + e[2] + e[3];
        const float q = expf(sqrtf(r1.z * r1.z + r1.w * r1.w));
        o[3] = S / (1.f + q);
        o[4] = S / (1.f + q) * q;
        o[6] = 0.5f * atan2f(r1.z, r1.w);
    }
#pragma unroll
    for (int c = 0; c < 7; ++c) box[i * 7 + c] = o[c];
}
__global__ __launch_bounds__(256) void box_decode7_bwd_k(const float* __restrict__ raw, const float* __restrict__ dbox, const uint8_t* __restrict__ yaw,
                                                         int64_t M, float* __restrict__ draw) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    const float4 r0 = reinterpret_cast<const float4*>(raw + i * 8)[0], r1 = reinterpret_cast<const float4*>(raw + i * 8)[1];
    const float e[6] = {expf(r0.x), expf(r0.y), expf(r0.z), expf(r0.w), expf(r1.x), expf(r1.y)};
    float d[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) d[c] = dbox[i * 7 + c];
    float de[6], g6 = 0.f, g7 = 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a) { de[2 * a] = -d[a] / 2; de[2 * a + 1] = d[a] / 2; }      // centre_a = c_a + (e_{2a+1} - e_{2a}) / 2
    de[4] += d[5]; de[5] += d[5];                                                          // size_z = e4 + e5
    if (!yaw || yaw[i]) {
        const float a6 = r1.z, a7 = r1.w, rho2 = a6 * a6 + a7 * a7, rho = sqrtf(rho2);
        const float q = expf(rho), S = e[0] + e[1] + e[2] + e[3], inv = 1.f / (1.f + q);
        const float dS = (d[3] + d[4] * q) * inv;                  // w = S / (1 + q), l = S q / (1 + q)
        const float dq = (d[4] - d[3]) * S * inv * inv;
#pragma unroll
        for (int c = 0; c < 4; ++c) de[c] += dS;
        if (rho2 > 0.f) {                                          // (rho = 0: torch's sqrt / atan2 backward is 0 * inf there; no gradient is the usable answer)
            const float drho = dq * q;
            g6 = drho * a6 / rho + 0.5f * d[6] * a7 / rho2;        // d atan2(y = a6, x = a7): dy = x / (x^2 + y^2), dx = -y / (x^2 + y^2)
            g7 = drho * a7 / rho - 0.5f * d[6] * a6 / rho2;
        }
    } else {
        de[0] += d[3]; de[1] += d[3]; de[2] += d[4]; de[3] += d[4];          // size_x = e0 + e1, size_y = e2 + e3
    }
    reinterpret_cast<float4*>(draw + i * 8)[0] = make_float4(e[0] * de[0], e[1] * de[1], e[2] * de[2], e[3] * de[3]);
    reinterpret_cast<float4*>(draw + i * 8)[1] = make_float4(e[4] * de[4], e[5] * de[5], g6, g7);
}

}  // namespace u3d

using namespace u3d;

extern "C" {

int u3d_box_decode_fwd(const float* raw, const float* centers, int64_t M, float* box, u3d_stream_t stream) {
    if (!raw || !centers || !box || M < 0) return U3D_EINVAL;
    if (M == 0) return U3D_OK;
    hipLaunchKernelGGL(box_decode_fwd_k, dim3((unsigned)ceil_div(M, 256)), dim3(256), 0, (hipStream_t)stream, raw, centers, M, box);
    return check_launch("box_decode_fwd");
}

int u3d_box_decode_bwd(const float* raw, const float* dbox, int64_t M, float* draw, u3d_stream_t stream) {
    if (!raw || !dbox || !draw || M < 0) return U3D_EINVAL;
    if (M == 0) return U3D_OK;
    hipLaunchKernelGGL(box_decode_bwd_k, dim3((unsigned)ceil_div(M, 256)), dim3(256), 0, (hipStream_t)stream, raw, dbox, M, draw);
    return check_launch("box_decode_bwd");
}

int u3d_box_decode7_fwd(const float* raw, const float* centers, const uint8_t* yaw_rows, int64_t M, float* box, u3d_stream_t stream) {
    if (!raw || !centers || !box || M < 0) return U3D_EINVAL;
    if (M == 0) return U3D_OK;
    hipLaunchKernelGGL(box_decode7_fwd_k, dim3((unsigned)ceil_div(M, 256)), dim3(256), 0, (hipStream_t)stream, raw, centers, yaw_rows, M, box);
    return check_launch("box_decode7_fwd");
}

int u3d_box_decode7_bwd(const float* raw, const float* dbox, const uint8_t* yaw_rows, int64_t M, float* draw, u3d_stream_t stream) {
    if (!raw || !dbox || !draw || M < 0) return U3D_EINVAL;
    if (M == 0) return U3D_OK;
    hipLaunchKernelGGL(box_decode7_bwd_k, dim3((unsigned)ceil_div(M, 256)), dim3(256), 0, (hipStream_t)stream, raw, dbox, yaw_rows, M, draw);
    return check_launch("box_decode7_bwd");
}

static inline int64_t al64(int64_t x) { return (x + 63) & ~(int64_t)63; }

static inline int crit_words(int max_gt) { return max_gt > 64 ? (max_gt + 63) / 64 : 1; }

// 0 = by the batch (pair-parallel cost kernel when max_gt > 64), 1 = always the per-query kernel, 2 = always the pair kernel.
// Host state for A/B timing (tools/criterion_time.py); both kernels evaluate the same expression per entry.
static int crit_cost_mode() {
    static const int mode = [] {
        const char* e = getenv("U3D_CRITERION_COST");
        return !e ? 0 : (!strcmp(e, "query") ? 1 : (!strcmp(e, "pair") ? 2 : 0));
    }();
    return mode;
}

int64_t u3d_criterion_ws_bytes_gt(int L, int B, int64_t n_tot, int64_t G, int64_t P, int max_gt) {
    if (L <= 0 || B <= 0 || n_tot < 0 || G < 0 || P < 0 || max_gt < 0) return U3D_EINVAL;
    return al64((int64_t)L * P * 4) + al64((int64_t)L * n_tot * 4) + al64((int64_t)L * G * 4) +
           al64((int64_t)L * n_tot * 8 * crit_words(max_gt)) + al64((int64_t)L * B * 16) + al64((int64_t)L * 8) +
           al64((int64_t)L * n_tot * 8) + 256;
}

int64_t u3d_criterion_ws_bytes(int L, int B, int64_t n_tot, int64_t G, int64_t P) {      // max_gt <= 64: one word per query
    return u3d_criterion_ws_bytes_gt(L, B, n_tot, G, P, 64);
}

int u3d_criterion_packed(const float* cls, const float* box, const int32_t* cu, const int32_t* gt_off, const int64_t* gt_labels,
                         const float* gt_boxes, const uint8_t* qmask, const int64_t* qm_off, const int32_t* scene_meta,
                         const float* scene_w, const int32_t* cidx, int L, int B, int64_t n_tot, int CU, int BD, int64_t G, int64_t P,
                         int max_gt, int min_query_slack, float w_cls, float w_box, float non_obj_w, float lw_cls, float lw_box,
                         float* loss, float* dcls, float* dbox, void* ws, u3d_stream_t stream) {
    if (!cls || !box || !cu || !gt_off || !qm_off || !scene_meta || !scene_w || !loss || !dcls || !dbox || !ws || L <= 0 || B <= 0 ||
        n_tot <= 0 || CU < 2 || (BD != 6 && BD != 7) || G < 0 || P < 0)
        return U3D_EINVAL;
    if (G > 0 && (!gt_labels || !gt_boxes || !qmask)) return U3D_EINVAL;
    if (max_gt < 0 || max_gt > G) { set_error("criterion: max_gt %d is not in [0, G = %lld]", max_gt, (long long)G); return U3D_EINVAL; }
    if (L > 65535) { set_error("criterion: %d layers exceed the 65535 rows of the launch grid", L); return U3D_EUNSUPPORTED; }
    // What bounds a scene is 32-bit indexing: queries, GTs and the (query, GT) entries of one scene are counted in int.  The scene
    // sizes themselves live in device arrays; n_tot * max_gt and P bound every scene's n_b * g_b from above.
    {
        const int64_t lim = 0x7fffffff;
        const int64_t pairs = P < n_tot * (int64_t)max_gt ? P : n_tot * (int64_t)max_gt;
        if (n_tot > lim || G > lim || pairs > lim || (int64_t)L * G > lim) {
            set_error("criterion: the scene with the most ground truth (max_gt %d of G %lld boxes, n_tot %lld queries, P %lld entries, "
                      "L %d) may hold up to %lld (query, GT) entries: beyond the 32-bit index range of the kernels",
                      max_gt, (long long)G, (long long)n_tot, (long long)P, L, (long long)pairs);
            return U3D_EUNSUPPORTED;
        }
    }
    if (G > 0 && min_query_slack < 0) {        // torch.topk(cost, topk + 1, dim=0) of the reference raises here as well
        set_error("criterion: a scene with ground truth has fewer queries than its topk + 1 (slack %d)", min_query_slack);
        return U3D_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    CritParams p;
    p.cls = cls; p.box = box; p.cu = cu; p.gt_off = gt_off; p.gt_labels = gt_labels; p.gt_boxes = gt_boxes; p.qmask = qmask; p.qm_off = qm_off;
    p.meta = scene_meta; p.scene_w = scene_w; p.cidx = cidx;
    p.L = L; p.B = B; p.CU = CU; p.BD = BD; p.n_tot = n_tot; p.G = G; p.P = P;
    p.W = crit_words(max_gt);
    p.w_cls = w_cls; p.w_box = w_box; p.non_obj_w = non_obj_w; p.lw_cls = lw_cls; p.lw_box = lw_box;
    char* w = (char*)ws;
    p.cost = (float*)w; w += al64((int64_t)L * P * 4);
    p.logz = (float*)w; w += al64((int64_t)L * n_tot * 4);
    p.kth = (float*)w; w += al64((int64_t)L * G * 4);
    p.mm = (unsigned long long*)w; w += al64((int64_t)L * n_tot * 8 * p.W);
    p.stats = (float*)w; w += al64((int64_t)L * B * 16);
    p.scale = (float*)w; w += al64((int64_t)L * 8);
    p.mxse = (float*)w;
    p.loss = loss; p.dcls = dcls; p.dbox = dbox;
    const unsigned gq = (unsigned)ceil_div((int64_t)L * n_tot, 256);
    const int mode = crit_cost_mode();
    if (mode == 2 || (mode == 0 && max_gt > 64)) {
        hipLaunchKernelGGL(crit_lse_k, dim3(gq), dim3(256), 0, s, p);
        if (P > 0) hipLaunchKernelGGL(crit_cost_pair_k, dim3((unsigned)ceil_div(P, 64), (unsigned)L), dim3(64), 0, s, p);
    } else {
        hipLaunchKernelGGL(crit_cost_k, dim3(gq), dim3(256), 0, s, p);
    }
    if (G > 0) hipLaunchKernelGGL(crit_kth_k, dim3((unsigned)((int64_t)L * G)), dim3(64), 0, s, p);
    hipLaunchKernelGGL(crit_stats_k, dim3((unsigned)(L * B)), dim3(256), 0, s, p);
    hipLaunchKernelGGL(crit_final_k, dim3(1), dim3(1), 0, s, p);
    if (p.W > 1) hipLaunchKernelGGL(crit_grad_k<true>, dim3(gq), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(crit_grad_k<false>, dim3(gq), dim3(256), 0, s, p);
    return check_launch("criterion_packed");
}

}  // extern "C"
