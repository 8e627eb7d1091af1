// K-aug: the training-input pipeline of a whole ragged batch on the device (unidet3d/transforms_3d.py, unidet3d/loading.py:71-107 and
// mmdet3d's RandomFlip3D / GlobalRotScaleTrans after file loading):
//   * point map      -- row gather (PointSample_), per-scene float32 affine (flip, rotation, scale, translation), colour
//                       normalisation and the voxel-unit coordinates ElasticTransfrom starts from, one launch;
//   * extent         -- per scene and axis max |coord| (float32 / float64 input), exact: integer atomic max of the bit patterns;
//   * noise blur     -- the six zero-padded 3-tap sweeps of every scene's three noise grids, one launch per sweep;
//   * elastic apply  -- float64 trilinear lookup of the blurred grids per point (transforms.trilinear_lookup's formula and corner order);
//   * dense relabel  -- np.unique(ids, return_inverse / return_index) per scene: presence marks, exclusive scan, map;
//   * superpoint masks -- integer histograms over (instance, superpoint) and (superpoint), 2 hits > cnt.
// The batch is the concatenated per-point arrays plus [B+1] point offsets; no launch is per scene or per channel.  Results are
// defined by operation order (this file is built with -ffp-contract=off); no floating-point atomic is issued.
#include <math.h>

#include "u3d_common.h"

namespace u3d {

// scene of batch element i: the b in [0, B) with off[b] <= i < off[b+1] (empty scenes are skipped); i < off[B]
__device__ __forceinline__ int aug_scene_of(const int64_t* __restrict__ off, int B, int64_t i, int64_t mul = 1) {
    int lo = 0, hi = B;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] * mul <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// row of the source arrays that batch point (b, local) reads: src [B][2] = (first row, row count) of the scene in the cache;
// gather (nullable) holds a non-negative draw per batch point, reduced modulo the scene's row count (indices below the count are
// taken as they are).  -1: nothing to read (empty source scene / outside the source arrays).
__device__ __forceinline__ int64_t aug_src_row(const int64_t* __restrict__ src, const int64_t* __restrict__ gather, int b, int64_t i,
                                               int64_t local, int64_t src_rows) {
    const int64_t first = src[2 * b], cnt = src[2 * b + 1];
    if (cnt <= 0 || first < 0) return -1;
    const int64_t l = gather ? (int64_t)((uint64_t)gather[i] % (uint64_t)cnt) : (local < cnt ? local : cnt - 1);
    const int64_t row = first + l;
    return row < src_rows ? row : -1;
}

// ---------------------------------------------------------------------------------------------------------------- point map
// DN: DenormalizePointsColor first (flags bit 3: c * dstd, bit 2: + dmean), then the normalisation; DN = false is the kernel
// u3d_aug_points has always launched
struct AugDenorm { float m0, m1, m2, s0, s1, s2; };

template <bool DN>
__global__ __launch_bounds__(256) void aug_points_k(const float* __restrict__ srcp, const int64_t* __restrict__ gather,
                                                    const int64_t* __restrict__ src, const int64_t* __restrict__ off, int B, int64_t n,
                                                    int64_t src_rows, const float* __restrict__ aff, float m0, float m1, float m2, float s0,
                                                    float s1, float s2, int flags, float vs, float* __restrict__ pts,
                                                    float* __restrict__ coords, AugDenorm dn) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int b = aug_scene_of(off, B, i);
    const int64_t row = aug_src_row(src, gather, b, i, i - off[b], src_rows);
    float x = 0.f, y = 0.f, z = 0.f, r = 0.f, g = 0.f, bl = 0.f;
    if (row >= 0) {
        const float2* p = reinterpret_cast<const float2*>(srcp + row * 6);       // rows are 24 bytes: 8-byte aligned
        const float2 a0 = p[0], a1 = p[1], a2 = p[2];
        x = a0.x; y = a0.y; z = a1.x; r = a1.y; g = a2.x; bl = a2.y;
    }
    const float* a = aff + (int64_t)b * 12;
    const float xo = ((a[0] * x + a[1] * y) + a[2] * z) + a[3];
    const float yo = ((a[4] * x + a[5] * y) + a[6] * z) + a[7];
    const float zo = ((a[8] * x + a[9] * y) + a[10] * z) + a[11];
    if (DN) {
        if (flags & 8) { r = r * dn.s0; g = g * dn.s1; bl = bl * dn.s2; }
        if (flags & 4) { r = r + dn.m0; g = g + dn.m1; bl = bl + dn.m2; }
    }
    if (flags & 1) { r = r - m0; g = g - m1; bl = bl - m2; }
    if (flags & 2) { r = r / s0; g = g / s1; bl = bl / s2; }
    float2* o = reinterpret_cast<float2*>(pts + i * 6);
    o[0] = make_float2(xo, yo); o[1] = make_float2(zo, r); o[2] = make_float2(g, bl);
    if (coords) {
        coords[i * 3 + 0] = xo / vs; coords[i * 3 + 1] = yo / vs; coords[i * 3 + 2] = zo / vs;
    }
}

// ---------------------------------------------------------------------------------------------------------------- boxes
// one thread per box of the batch: rows (cx, cy, cz, dx, dy, dz, yaw) of the cache -> the same row after the scene's flip / rotation /
// scale / translation.  Centre: the point map's expression; size: size * float(scale); yaw in fp64 (flip_h: pi - yaw, flip_v: -yaw,
// + angle), rounded once, no period wrapping.  scal [B][4] = (flip_h, flip_v, angle, scale); scenes with with_yaw[b] == 0 keep yaw 0.
__global__ __launch_bounds__(256) void aug_boxes_k(const float* __restrict__ srcb, int64_t src_rows, const int64_t* __restrict__ bsrc,
                                                   const int64_t* __restrict__ boff, int B, int64_t n, const float* __restrict__ aff,
                                                   const double* __restrict__ scal, const uint8_t* __restrict__ with_yaw,
                                                   float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int b = aug_scene_of(boff, B, i);
    const int64_t row = aug_src_row(bsrc, nullptr, b, i, i - boff[b], src_rows);
    float v[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (row >= 0) {
#pragma unroll
        for (int k = 0; k < 7; ++k) v[k] = srcb[row * 7 + k];
    }
    const float* a = aff + (int64_t)b * 12;
    const double* sc = scal + (int64_t)b * 4;
    const float s = (float)sc[3];
    float* o = out + i * 7;
    o[0] = ((a[0] * v[0] + a[1] * v[1]) + a[2] * v[2]) + a[3];
    o[1] = ((a[4] * v[0] + a[5] * v[1]) + a[6] * v[2]) + a[7];
    o[2] = ((a[8] * v[0] + a[9] * v[1]) + a[10] * v[2]) + a[11];
    o[3] = v[3] * s; o[4] = v[4] * s; o[5] = v[5] * s;
    float yo = 0.f;
    if (with_yaw[b]) {
        double y = (double)v[6];
        if (sc[0] != 0.0) y = 3.14159265358979323846 - y;
        if (sc[1] != 0.0) y = -y;
        y = y + sc[2];
        yo = (float)y;
    }
    o[6] = yo;
}

// ---------------------------------------------------------------------------------------------------------------- extent
constexpr int EXT_PER_THREAD = 8;

__device__ __forceinline__ void aug_atomic_max_bits(float* p, float v) { atomicMax(reinterpret_cast<unsigned int*>(p), __float_as_uint(v)); }
__device__ __forceinline__ void aug_atomic_max_bits(double* p, double v) {
    atomicMax(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__double_as_longlong(v));
}

// non-negative IEEE values order like their bit patterns: the integer atomic max of the bits is the exact maximum; out is zeroed
template <typename T>
__global__ __launch_bounds__(256) void aug_extent_k(const T* __restrict__ x, const int64_t* __restrict__ off, T* __restrict__ out) {
    __shared__ T red[3][4];
    const int b = blockIdx.y;
    const int64_t lo = off[b], cnt = off[b + 1] - lo;
    const int64_t start = (int64_t)blockIdx.x * 256 * EXT_PER_THREAD;
    if (start >= cnt) return;                         // uniform per block
    T m[3] = {0, 0, 0};
    for (int k = 0; k < EXT_PER_THREAD; ++k) {
        const int64_t l = start + (int64_t)k * 256 + threadIdx.x;
        if (l < cnt) {
            const T* p = x + (lo + l) * 3;
#pragma unroll
            for (int d = 0; d < 3; ++d) { const T v = fabs(p[d]); if (v > m[d]) m[d] = v; }
        }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        for (int s = 32; s > 0; s >>= 1) { const T o = __shfl_down(m[d], s, 64); if (o > m[d]) m[d] = o; }
        if ((threadIdx.x & 63) == 0) red[d][threadIdx.x >> 6] = m[d];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int d = threadIdx.x;
        T v = red[d][0];
        for (int w = 1; w < 4; ++w) if (red[d][w] > v) v = red[d][w];
        aug_atomic_max_bits(out + b * 3 + d, v);
    }
}

template <typename T>
static int aug_extent(const T* x, const int64_t* off, int B, int64_t max_pts, T* out, hipStream_t s, const char* what) {
    if (B < 0 || max_pts < 0) return U3D_EINVAL;
    if (B > 0 && (!off || !out)) return U3D_EINVAL;
    if (B == 0) return U3D_OK;
    if (hipMemsetAsync(out, 0, sizeof(T) * 3 * B, s) != hipSuccess) { set_error("%s: memset failed", what); return U3D_ELAUNCH; }
    if (max_pts == 0) return U3D_OK;
    if (!x) return U3D_EINVAL;
    const int64_t chunks = ceil_div(max_pts, 256 * EXT_PER_THREAD);
    if (chunks > 0x7fffffff || B > 65535) { set_error("%s: batch too large", what); return U3D_EINVAL; }
    hipLaunchKernelGGL(aug_extent_k<T>, dim3((unsigned)chunks, B), dim3(256), 0, s, x, off, out);
    return check_launch(what);
}

// ---------------------------------------------------------------------------------------------------------------- noise blur
// one sweep of _box_blur3 along `axis` over every scene's [3][d0][d1][d2] grids (scene b at floats 3 goff[b] .. 3 goff[b+1]);
// last = 1 writes the cell-major form the elastic kernel reads: float4 (channel 0, 1, 2, unused) per cell at cell goff[b] + r
__global__ __launch_bounds__(256) void aug_blur_k(const float* __restrict__ in, float* __restrict__ out, const int32_t* __restrict__ dims,
                                                  const int64_t* __restrict__ goff, int B, int64_t total, int axis, int last) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int b = aug_scene_of(goff, B, e, 3);
    const int64_t d1 = dims[b * 3 + 1], d2 = dims[b * 3 + 2];
    const int64_t cells = goff[b + 1] - goff[b];
    const int64_t local = e - 3 * goff[b];
    const int64_t c = local / cells, r = local - c * cells;
    int64_t pos, len, stride;
    if (axis == 0) { pos = r / (d1 * d2); len = dims[b * 3]; stride = d1 * d2; }
    else if (axis == 1) { pos = (r / d2) % d1; len = d1; stride = d2; }
    else { pos = r % d2; len = d2; stride = 1; }
    const float third = (float)(1.0 / 3.0);
    const int64_t lo = 3 * goff[b], hi = 3 * goff[b + 1];                       // (dims that disagree with the offsets never read outside the scene)
    const float a = pos > 0 && e - stride >= lo ? in[e - stride] : 0.f, m = in[e], z = pos < len - 1 && e + stride < hi ? in[e + stride] : 0.f;
    const float v = (a * third + m * third) + z * third;
    if (last) out[(goff[b] + r) * 4 + c] = v; else out[e] = v;
}

// ---------------------------------------------------------------------------------------------------------------- elastic apply
__global__ __launch_bounds__(256) void aug_elastic_k(const void* __restrict__ xin, int in64, void* __restrict__ xout, int out64,
                                                     const int64_t* __restrict__ off, int B, int64_t n, const float4* __restrict__ grids,
                                                     const int64_t* __restrict__ goff, const int32_t* __restrict__ dims,
                                                     const uint8_t* __restrict__ gate, double gran, double mag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int b = aug_scene_of(off, B, i);
    double x[3];
#pragma unroll
    for (int d = 0; d < 3; ++d)
        x[d] = in64 ? static_cast<const double*>(xin)[i * 3 + d] : (double)static_cast<const float*>(xin)[i * 3 + d];
    double val[3] = {0.0, 0.0, 0.0};
    const int64_t d0 = dims[b * 3], d1 = dims[b * 3 + 1], d2 = dims[b * 3 + 2];
    if (gate[b] && d0 >= 2 && d1 >= 2 && d2 >= 2 && goff[b + 1] - goff[b] >= d0 * d1 * d2) {
        const int64_t dd[3] = {d0, d1, d2};
        double f[3];
        int64_t i0[3];
        bool inside = true;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double bd = (double)dd[d];
            const double t = (x[d] + (bd - 1) * gran) / (2.0 * gran);                 // fractional node index
            inside = inside && (t >= 0) && (t <= bd - 1);
            i0[d] = (int64_t)fmin(fmax(floor(t), 0.0), (double)(dd[d] - 2));
            f[d] = t - (double)i0[d];
        }
        if (inside) {
            const float4* g = grids + goff[b];
            double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const double wx = dx ? f[0] : 1 - f[0];
#pragma unroll
                for (int dy = 0; dy < 2; ++dy) {
                    const double wy = dy ? f[1] : 1 - f[1];
#pragma unroll
                    for (int dz = 0; dz < 2; ++dz) {
                        const double wz = dz ? f[2] : 1 - f[2];
                        const float4 q = g[((i0[0] + dx) * d1 + (i0[1] + dy)) * d2 + (i0[2] + dz)];
                        const double w = (wx * wy) * wz;
                        acc[0] = acc[0] + (double)q.x * w; acc[1] = acc[1] + (double)q.y * w; acc[2] = acc[2] + (double)q.z * w;
                    }
                }
            }
            val[0] = acc[0]; val[1] = acc[1]; val[2] = acc[2];
        }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double r = gate[b] ? x[d] + val[d] * mag : x[d];
        if (out64) static_cast<double*>(xout)[i * 3 + d] = r; else static_cast<float*>(xout)[i * 3 + d] = (float)r;
    }
}

// ---------------------------------------------------------------------------------------------------------------- dense relabel
// table slot of id v of scene b: v + 1 (slot 0 = id -1); ids outside [-1, table size - 2] are taken as -1
__global__ __launch_bounds__(256) void aug_relabel_mark_k(const int64_t* __restrict__ ids, const int64_t* __restrict__ gather,
                                                          const int64_t* __restrict__ src, const int64_t* __restrict__ off, int B, int64_t n,
                                                          int64_t src_rows, const int64_t* __restrict__ toff, const int64_t* __restrict__ sem,
                                                          const uint8_t* __restrict__ drop, int n_drop, int64_t* __restrict__ new_ids,
                                                          int64_t* __restrict__ sem_out, int32_t* __restrict__ marks,
                                                          int32_t* __restrict__ firstl) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int b = aug_scene_of(off, B, i);
    const int64_t local = i - off[b];
    const int64_t row = aug_src_row(src, gather, b, i, local, src_rows);
    int64_t id = row >= 0 ? ids[row] : -1;
    if (sem) {
        const int64_t sv = row >= 0 ? sem[row] : 0;
        if (drop && sv >= 0 && sv < n_drop && drop[sv]) id = -1;
        if (sem_out) sem_out[i] = sv;
    }
    const int64_t size = toff[b + 1] - toff[b];
    int64_t slot = id + 1;
    if (slot < 0 || slot >= size) slot = 0;
    new_ids[i] = slot;
    if (size > 0) {
        marks[toff[b] + slot] = 1;
        atomicMin(&firstl[toff[b] + slot], (int)local);
    }
}

// one workgroup per scene: exclusive scan of the presence marks -> rank of every present id; counts[b] = distinct ranked ids;
// first (nullable): batch row of the first occurrence of the id ranked r at first[toff[b] + r], 0 past the count
__global__ __launch_bounds__(256) void aug_relabel_scan_k(const int32_t* __restrict__ marks, const int32_t* __restrict__ firstl,
                                                          const int64_t* __restrict__ off, const int64_t* __restrict__ toff, int keep_negative,
                                                          int32_t* __restrict__ rank, int32_t* __restrict__ counts, int64_t* __restrict__ first) {
    __shared__ int wsum[4];
    __shared__ int base;
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t t0 = toff[b], size = toff[b + 1] - t0;
    if (t == 0) base = 0;
    if (keep_negative && size > 0 && t == 0) rank[t0] = -1;
    __syncthreads();
    for (int64_t s0 = keep_negative ? 1 : 0; s0 < size; s0 += 256) {
        // the marks are 0 / 1: a wave's prefix is a popcount of its ballot, the four waves meet through LDS (two barriers per 256 slots)
        const int64_t slot = s0 + t;
        const int mk = slot < size ? marks[t0 + slot] : 0;
        const unsigned long long bal = __ballot(mk != 0);
        if (lane == 0) wsum[w] = __popcll(bal);
        __syncthreads();
        int before = 0, all = 0;
        for (int k = 0; k < 4; ++k) { if (k < w) before += wsum[k]; all += wsum[k]; }
        const int r = base + before + __popcll(bal & ((1ull << lane) - 1ull));
        if (mk) {
            rank[t0 + slot] = r;
            if (first) first[t0 + r] = off[b] + firstl[t0 + slot];
        }
        __syncthreads();
        if (t == 0) base += all;
        __syncthreads();
    }
    const int total = base;
    if (t == 0) counts[b] = total;
    if (first)
        for (int64_t r = total + t; r < size; r += 256) first[t0 + r] = 0;
}

__global__ __launch_bounds__(256) void aug_relabel_map_k(const int64_t* __restrict__ off, int B, int64_t n, const int64_t* __restrict__ toff,
                                                         const int32_t* __restrict__ rank, int64_t* __restrict__ new_ids) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int b = aug_scene_of(off, B, i);
    new_ids[i] = toff[b + 1] > toff[b] ? (int64_t)rank[toff[b] + new_ids[i]] : -1;
}

__global__ __launch_bounds__(256) void aug_remap_k(int64_t* __restrict__ ids, const int64_t* __restrict__ off, int B, int64_t n,
                                                   const int64_t* __restrict__ table, const int64_t* __restrict__ toff) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int b = aug_scene_of(off, B, i);
    const int64_t id = ids[i];
    ids[i] = id >= 0 && id < toff[b + 1] - toff[b] ? table[toff[b] + id] : -1;
}

// ---------------------------------------------------------------------------------------------------------------- superpoint masks
__global__ __launch_bounds__(256) void aug_sp_hist_k(const int64_t* __restrict__ inst, const int64_t* __restrict__ sp,
                                                     const int64_t* __restrict__ src, int64_t src_rows, const int64_t* __restrict__ off, int B,
                                                     int64_t n, const int32_t* __restrict__ n_inst, const int64_t* __restrict__ sp_off,
                                                     const int64_t* __restrict__ mask_off, int32_t* __restrict__ hits, int32_t* __restrict__ cnt) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int b = aug_scene_of(off, B, i);
    int64_t row = i;
    if (src) row = aug_src_row(src, nullptr, b, i, i - off[b], src_rows);
    if (row < 0) return;
    const int64_t S = sp_off[b + 1] - sp_off[b], s = sp[row];
    if (s < 0 || s >= S) return;
    atomicAdd(&cnt[sp_off[b] + s], 1);
    const int64_t j = inst[i];
    if (j >= 0 && j < n_inst[b] && mask_off[b] + j * S + s < mask_off[b + 1]) atomicAdd(&hits[mask_off[b] + j * S + s], 1);
}

__global__ __launch_bounds__(256) void aug_sp_fin_k(const int64_t* __restrict__ sp_off, const int64_t* __restrict__ mask_off, int B, int64_t total,
                                                    const int32_t* __restrict__ hits, const int32_t* __restrict__ cnt, uint8_t* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int b = aug_scene_of(mask_off, B, e);
    const int64_t S = sp_off[b + 1] - sp_off[b];
    const int64_t s = (e - mask_off[b]) % S;
    out[e] = 2 * hits[e] > cnt[sp_off[b] + s] ? 1 : 0;
}

static inline int64_t align256(int64_t v) { return (v + 255) / 256 * 256; }
static inline bool grid_ok(int64_t n) { return ceil_div(n, 256) <= 0x7fffffff; }

}  // namespace u3d

using namespace u3d;

extern "C" {

static int aug_points_launch(const float* src_points, int64_t src_rows, const int64_t* gather, const int64_t* src, const int64_t* pt_offsets,
                             int B, int64_t n, const float* affine, const float* m, const float* sd, const float* dm, const float* dsd,
                             bool dn, float voxel_size, float* points, float* coords, u3d_stream_t stream) {
    if (B < 0 || n < 0 || src_rows < 0) return U3D_EINVAL;
    if (n == 0) return U3D_OK;
    if (B == 0 || !src_points || !src || !pt_offsets || !affine || !points || !grid_ok(n)) return U3D_EINVAL;
    if (coords && !(voxel_size > 0.f)) { set_error("aug_points: voxel_size must be positive"); return U3D_EINVAL; }
    const AugDenorm d = {dm ? dm[0] : 0.f, dm ? dm[1] : 0.f, dm ? dm[2] : 0.f, dsd ? dsd[0] : 1.f, dsd ? dsd[1] : 1.f, dsd ? dsd[2] : 1.f};
    const int flags = (m ? 1 : 0) | (sd ? 2 : 0) | (dm ? 4 : 0) | (dsd ? 8 : 0);
    hipLaunchKernelGGL(dn ? aug_points_k<true> : aug_points_k<false>, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream,
                       src_points, gather, src, pt_offsets, B, n, src_rows, affine, m ? m[0] : 0.f, m ? m[1] : 0.f, m ? m[2] : 0.f,
                       sd ? sd[0] : 1.f, sd ? sd[1] : 1.f, sd ? sd[2] : 1.f, flags, voxel_size, points, coords, d);
    return check_launch("aug_points");
}

int u3d_aug_points(const float* src_points, int64_t src_rows, const int64_t* gather, const int64_t* src, const int64_t* pt_offsets, int B,
                   int64_t n, const float* affine, const float* color_mean_host, const float* color_std_host, float voxel_size,
                   float* points, float* coords, u3d_stream_t stream) {
    return aug_points_launch(src_points, src_rows, gather, src, pt_offsets, B, n, affine, color_mean_host, color_std_host, nullptr, nullptr,
                             false, voxel_size, points, coords, stream);
}

int u3d_aug_points_dn(const float* src_points, int64_t src_rows, const int64_t* gather, const int64_t* src, const int64_t* pt_offsets, int B,
                      int64_t n, const float* affine, const float* color_mean_host, const float* color_std_host,
                      const float* denorm_mean_host, const float* denorm_std_host, float voxel_size, float* points, float* coords,
                      u3d_stream_t stream) {
    return aug_points_launch(src_points, src_rows, gather, src, pt_offsets, B, n, affine, color_mean_host, color_std_host, denorm_mean_host,
                             denorm_std_host, true, voxel_size, points, coords, stream);
}

int u3d_aug_boxes(const float* src_boxes, int64_t src_rows, const int64_t* box_src, const int64_t* box_offsets, int B, int64_t n,
                  const float* affine, const double* scalars, const uint8_t* with_yaw, float* boxes, u3d_stream_t stream) {
    if (B < 0 || n < 0 || src_rows < 0) return U3D_EINVAL;
    if (n == 0) return U3D_OK;
    if (B == 0 || !src_boxes || !box_src || !box_offsets || !affine || !scalars || !with_yaw || !boxes || !grid_ok(n)) return U3D_EINVAL;
    hipLaunchKernelGGL(aug_boxes_k, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, src_boxes, src_rows, box_src, box_offsets,
                       B, n, affine, scalars, with_yaw, boxes);
    return check_launch("aug_boxes");
}

int u3d_aug_extent_f32(const float* coords, const int64_t* pt_offsets, int B, int64_t max_pts_per_scene, float* extent, u3d_stream_t stream) {
    return aug_extent<float>(coords, pt_offsets, B, max_pts_per_scene, extent, (hipStream_t)stream, "aug_extent_f32");
}

int u3d_aug_extent_f64(const double* coords, const int64_t* pt_offsets, int B, int64_t max_pts_per_scene, double* extent, u3d_stream_t stream) {
    return aug_extent<double>(coords, pt_offsets, B, max_pts_per_scene, extent, (hipStream_t)stream, "aug_extent_f64");
}

int64_t u3d_aug_noise_blur_ws_bytes(int64_t total_cells) { return total_cells < 0 ? -1 : 2 * align256(3 * total_cells * 4); }

int u3d_aug_noise_blur(const float* noise, const int32_t* dims, const int64_t* grid_offsets, int B, int64_t total_cells, float* grids,
                       void* ws, u3d_stream_t stream) {
    if (B < 0 || total_cells < 0) return U3D_EINVAL;
    if (total_cells == 0) return U3D_OK;
    if (B == 0 || !noise || !dims || !grid_offsets || !grids || !ws || !grid_ok(3 * total_cells)) return U3D_EINVAL;
    float* bufA = static_cast<float*>(ws);
    float* bufB = reinterpret_cast<float*>(static_cast<char*>(ws) + align256(3 * total_cells * 4));
    const float* in = noise;
    const int64_t total = 3 * total_cells;
    for (int k = 0; k < 6; ++k) {                            // axes 0, 1, 2, 0, 1, 2
        float* out = k == 5 ? grids : (k & 1 ? bufB : bufA);
        hipLaunchKernelGGL(aug_blur_k, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, in, out, dims, grid_offsets, B,
                           total, k % 3, k == 5 ? 1 : 0);
        in = out;
    }
    return check_launch("aug_noise_blur");
}

int u3d_aug_elastic(const void* coords_in, int in_f64, void* coords_out, int out_f64, const int64_t* pt_offsets, int B, int64_t n,
                    const float* grids, const int64_t* grid_offsets, const int32_t* dims, const uint8_t* gate, double gran, double mag,
                    u3d_stream_t stream) {
    if (B < 0 || n < 0) return U3D_EINVAL;
    if (n == 0) return U3D_OK;
    if (B == 0 || !coords_in || !coords_out || !pt_offsets || !grid_offsets || !dims || !gate || !grid_ok(n)) return U3D_EINVAL;
    if (!(gran > 0.0)) { set_error("aug_elastic: gran must be positive"); return U3D_EINVAL; }
    hipLaunchKernelGGL(aug_elastic_k, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, coords_in, in_f64, coords_out, out_f64,
                       pt_offsets, B, n, reinterpret_cast<const float4*>(grids), grid_offsets, dims, gate, gran, mag);
    return check_launch("aug_elastic");
}

int64_t u3d_relabel_ids_ws_bytes(int64_t table_entries) { return table_entries < 0 ? -1 : 3 * align256(table_entries * 4); }

int u3d_relabel_ids(const int64_t* ids, int64_t src_rows, const int64_t* gather, const int64_t* src, const int64_t* pt_offsets, int B, int64_t n,
                    const int64_t* table_offsets, int64_t table_entries, int keep_negative, const int64_t* sem, const uint8_t* sem_drop,
                    int n_sem_drop, int64_t* new_ids, int64_t* sem_out, int32_t* counts, int64_t* first, void* ws, u3d_stream_t stream) {
    if (B < 0 || n < 0 || src_rows < 0 || table_entries < 0 || n_sem_drop < 0) return U3D_EINVAL;
    if (B == 0) return n == 0 ? U3D_OK : U3D_EINVAL;
    if (!pt_offsets || !table_offsets || !counts || !ws || !grid_ok(n) || B > 0x7fffffff / 2) return U3D_EINVAL;
    if (n > 0 && (!ids || !src || !new_ids)) return U3D_EINVAL;
    if (n > 0x7fffffff) { set_error("relabel_ids: more than 2^31 points"); return U3D_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    const int64_t part = align256(table_entries * 4);
    int32_t* marks = static_cast<int32_t*>(ws);
    int32_t* firstl = reinterpret_cast<int32_t*>(static_cast<char*>(ws) + part);
    int32_t* rank = reinterpret_cast<int32_t*>(static_cast<char*>(ws) + 2 * part);
    if (table_entries > 0) {
        if (hipMemsetAsync(marks, 0, table_entries * 4, s) != hipSuccess || hipMemsetAsync(firstl, 0x7f, table_entries * 4, s) != hipSuccess) {
            set_error("relabel_ids: memset failed");
            return U3D_ELAUNCH;
        }
    }
    if (n > 0)
        hipLaunchKernelGGL(aug_relabel_mark_k, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, ids, gather, src, pt_offsets, B, n, src_rows,
                           table_offsets, sem, sem_drop, n_sem_drop, new_ids, sem_out, marks, firstl);
    hipLaunchKernelGGL(aug_relabel_scan_k, dim3(B), dim3(256), 0, s, marks, firstl, pt_offsets, table_offsets, keep_negative, rank, counts, first);
    if (n > 0)
        hipLaunchKernelGGL(aug_relabel_map_k, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, pt_offsets, B, n, table_offsets, rank, new_ids);
    return check_launch("relabel_ids");
}

int u3d_aug_remap_ids(int64_t* ids, const int64_t* pt_offsets, int B, int64_t n, const int64_t* table, const int64_t* table_offsets,
                      u3d_stream_t stream) {
    if (B < 0 || n < 0) return U3D_EINVAL;
    if (n == 0) return U3D_OK;
    if (B == 0 || !ids || !pt_offsets || !table || !table_offsets || !grid_ok(n)) return U3D_EINVAL;
    hipLaunchKernelGGL(aug_remap_k, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, ids, pt_offsets, B, n, table, table_offsets);
    return check_launch("aug_remap_ids");
}

int64_t u3d_aug_sp_masks_ws_bytes(int64_t mask_entries, int64_t n_superpoints) {
    return mask_entries < 0 || n_superpoints < 0 ? -1 : align256(mask_entries * 4) + align256(n_superpoints * 4);
}

int u3d_aug_sp_masks(const int64_t* inst, const int64_t* sp, const int64_t* sp_src, int64_t src_rows, const int64_t* pt_offsets, int B, int64_t n,
                     const int32_t* n_inst, const int64_t* sp_offsets, const int64_t* mask_offsets, int64_t mask_entries, int64_t n_superpoints,
                     uint8_t* masks, void* ws, u3d_stream_t stream) {
    if (B < 0 || n < 0 || mask_entries < 0 || n_superpoints < 0 || src_rows < 0) return U3D_EINVAL;
    if (mask_entries == 0) return U3D_OK;                 // no instance anywhere: every matrix is [0, S]
    if (B == 0 || !pt_offsets || !n_inst || !sp_offsets || !mask_offsets || !masks || !ws || !grid_ok(n) || !grid_ok(mask_entries))
        return U3D_EINVAL;
    if (n > 0 && (!inst || !sp)) return U3D_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    int32_t* hits = static_cast<int32_t*>(ws);
    int32_t* cnt = reinterpret_cast<int32_t*>(static_cast<char*>(ws) + align256(mask_entries * 4));
    if (hipMemsetAsync(ws, 0, align256(mask_entries * 4) + n_superpoints * 4, s) != hipSuccess) {
        set_error("aug_sp_masks: memset failed");
        return U3D_ELAUNCH;
    }
    if (n > 0)
        hipLaunchKernelGGL(aug_sp_hist_k, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, inst, sp, sp_src, src_rows, pt_offsets, B, n, n_inst,
                           sp_offsets, mask_offsets, hits, cnt);
    hipLaunchKernelGGL(aug_sp_fin_k, dim3((unsigned)ceil_div(mask_entries, 256)), dim3(256), 0, s, sp_offsets, mask_offsets, B, mask_entries, hits,
                       cnt, masks);
    return check_launch("aug_sp_masks");
}

}  // extern "C"
