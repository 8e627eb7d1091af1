// Optimizer tail of a training step: global gradient norm, clipping and decoupled-weight-decay AdamW over every parameter tensor
// of a model in two launches (one without clipping), driven by one device table of rows (include/u3d.h, "R15").
//
// Block b of either kernel belongs to the last row whose first block is <= b (the idiom of weight_pack_batch_k, spconv.hip) and
// covers elements [c CHUNK, (c + 1) CHUNK) of that row, c = b - first block.  Thread t owns the four-element groups t, t + 256,
// t + 512, t + 768 of the chunk in BOTH the 16-byte path (every pointer of the row 16-byte aligned: one dwordx4 access per group and
// array) and the dword path (anything else, and the group that straddles the end of a row), so the arithmetic per element -- and
// the order of every sum -- is the same whichever path serves a row.  Compiled with -ffp-contract=off (build.py).
//
// Reductions: squares of fp32 values are exact in fp64; a thread adds its squares in ascending element order, the block adds its
// threads with a fixed tree, U3D_OPTIM_PARTIALS blocks each own a contiguous run of chunks and write one partial; every block of
// the update kernel adds the partials with the same fixed tree (4 KiB of L2 reads against the 450 KiB the block streams).  No atomics.
#include "u3d_common.h"

namespace u3d {

constexpr int CHUNK = U3D_OPTIM_CHUNK;
constexpr int NPART = U3D_OPTIM_PARTIALS;
constexpr int THREADS = 256;
constexpr int GROUPS = CHUNK / (4 * THREADS);          // four-element groups per thread and chunk
static_assert(CHUNK % (4 * THREADS) == 0 && NPART == 2 * THREADS, "chunk / partial layout");

struct OptimRow {
    float* p;              // parameter
    const float* g;        // gradient (nullptr: the parameter is skipped this step)
    int64_t moff;          // offset of the row's moments in exp_avg / exp_avg_sq (floats, multiple of 4)
    int64_t numel;
    double lr, wd;
    int64_t lag;           // global steps this parameter has missed: its own step count is step - lag
    int64_t block0;        // first block
};
static_assert(sizeof(OptimRow) == 64, "OptimRow is eight 64-bit words (optim.py builds it as int64 [n][8])");

__device__ __forceinline__ int row_of_block(const OptimRow* __restrict__ rows, int n_rows, int64_t b) {
    int lo = 0, hi = n_rows;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (rows[mid].block0 <= b) lo = mid; else hi = mid;
    }
    return lo;
}

// elements [e, e + 4) of an array of n: one 16-byte access when allowed and whole, else dwords (absent elements read as 0)
template <bool VEC>
__device__ __forceinline__ void load4(const float* __restrict__ a, int64_t e, int64_t n, float (&out)[4]) {
    if (VEC && e + 4 <= n) {
        const float4 v = *reinterpret_cast<const float4*>(a + e);
        out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) out[i] = e + i < n ? a[e + i] : 0.f;
    }
}
template <bool VEC>
__device__ __forceinline__ void store4(float* __restrict__ a, int64_t e, int64_t n, const float (&in)[4]) {
    if (VEC && e + 4 <= n) {
        *reinterpret_cast<float4*>(a + e) = float4{in[0], in[1], in[2], in[3]};
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (e + i < n) a[e + i] = in[i];
    }
}

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// sh[0] = sum of the 256 values the threads hold, added as a fixed binary tree
__device__ __forceinline__ double block_tree_sum(double v, double* sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
#pragma unroll
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (t < s) sh[t] += sh[t + s];
        __syncthreads();
    }
    return sh[0];
}

template <bool VEC>
__device__ __forceinline__ double chunk_sumsq(const float* __restrict__ g, int64_t e0, int64_t numel, double acc) {
    float v[GROUPS][4];
#pragma unroll
    for (int k = 0; k < GROUPS; ++k) load4<VEC>(g, e0 + 4 * ((int64_t)threadIdx.x + k * THREADS), numel, v[k]);
#pragma unroll
    for (int k = 0; k < GROUPS; ++k)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc += (double)v[k][i] * (double)v[k][i];
    return acc;
}

// partials[j] = sum of squares of the gradient chunks [j per, (j + 1) per), per = ceil(total_blocks / NPART)
__global__ __launch_bounds__(THREADS) void optim_sumsq_k(const OptimRow* __restrict__ rows, int n_rows, int64_t total_blocks,
                                                         double* __restrict__ partials) {
    __shared__ double sh[THREADS];
    const int64_t per = (total_blocks + NPART - 1) / NPART;
    const int64_t c0 = (int64_t)blockIdx.x * per, c1 = c0 + per < total_blocks ? c0 + per : total_blocks;
    double acc = 0.0;
    if (c0 < c1) {
        int r = row_of_block(rows, n_rows, c0);
        for (int64_t c = c0; c < c1; ++c) {
            while (r + 1 < n_rows && rows[r + 1].block0 <= c) ++r;
            const float* g = rows[r].g;
            const int64_t numel = rows[r].numel, e0 = (c - rows[r].block0) * CHUNK;
            if (g == nullptr || e0 >= numel) continue;
            acc = aligned16(g) ? chunk_sumsq<true>(g, e0, numel, acc) : chunk_sumsq<false>(g, e0, numel, acc);
        }
    }
    const double s = block_tree_sum(acc, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__device__ __forceinline__ double powi(double b, int64_t t) {
    double r = 1.0;
    for (; t > 0; t >>= 1, b *= b)
        if (t & 1) r *= b;
    return r;
}

struct AdamScalars { double lr, lr_wd, beta1, beta2, one_m_beta1, one_m_beta2, eps; float step_size, bc2_sqrt, coef; };

// one element, in the operation order (and the mixed fp64 / fp32 evaluation) of torch's fused AdamW: the hyper-parameters are
// doubles, every assignment rounds once to fp32
template <bool CLIP>
__device__ __forceinline__ void adamw_element(float& p, float g, float& m, float& v, const AdamScalars& a) {
    if (CLIP) g = g * a.coef;
    if (a.lr_wd != 0.0) p = (float)((double)p - a.lr_wd * (double)p);
    m = (float)(a.beta1 * (double)m + a.one_m_beta1 * (double)g);
    v = (float)(a.beta2 * (double)v + a.one_m_beta2 * (double)g * (double)g);
    const float denom = (float)((double)(sqrtf(v) / a.bc2_sqrt) + a.eps);
    p = p - a.step_size * m / denom;
}

template <bool CLIP, bool VEC>
__device__ __forceinline__ void adamw_chunk(const OptimRow& r, int64_t e0, float* __restrict__ m_all, float* __restrict__ v_all,
                                            const AdamScalars& a) {
    float* __restrict__ pm = m_all + r.moff;
    float* __restrict__ pv = v_all + r.moff;
    float p[GROUPS][4], g[GROUPS][4], m[GROUPS][4], v[GROUPS][4];
#pragma unroll
    for (int k = 0; k < GROUPS; ++k) {
        const int64_t e = e0 + 4 * ((int64_t)threadIdx.x + k * THREADS);
        load4<VEC>(r.p, e, r.numel, p[k]);
        load4<VEC>(r.g, e, r.numel, g[k]);
        load4<VEC>(pm, e, r.numel, m[k]);
        load4<VEC>(pv, e, r.numel, v[k]);
    }
#pragma unroll
    for (int k = 0; k < GROUPS; ++k) {
        const int64_t e = e0 + 4 * ((int64_t)threadIdx.x + k * THREADS);
        if (e >= r.numel) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) adamw_element<CLIP>(p[k][i], g[k][i], m[k][i], v[k][i], a);
        store4<VEC>(r.p, e, r.numel, p[k]);
        store4<VEC>(pm, e, r.numel, m[k]);
        store4<VEC>(pv, e, r.numel, v[k]);
    }
}

template <bool CLIP>
__global__ __launch_bounds__(THREADS) void optim_adamw_k(const OptimRow* __restrict__ rows, int n_rows, float* __restrict__ m_all,
                                                         float* __restrict__ v_all, double beta1, double beta2, double eps, float max_norm,
                                                         int64_t step, const double* __restrict__ partials, float* __restrict__ total_norm) {
    AdamScalars a;
    a.coef = 1.f;
    if (CLIP) {
        __shared__ double sh[THREADS];
        const double total = block_tree_sum(partials[threadIdx.x] + partials[threadIdx.x + THREADS], sh);
        const float norm = (float)sqrt(total);
        const float c = max_norm / (norm + 1e-6f);
        a.coef = c < 1.f ? c : 1.f;            // (a NaN norm gives coef 1, the gradients carry it on)
        if (blockIdx.x == 0 && threadIdx.x == 0) *total_norm = norm;
    }
    const OptimRow r = rows[row_of_block(rows, n_rows, (int64_t)blockIdx.x)];
    const int64_t e0 = ((int64_t)blockIdx.x - r.block0) * CHUNK;
    if (r.g == nullptr || e0 >= r.numel) return;
    const int64_t t = step - r.lag;
    a.lr = r.lr; a.lr_wd = r.lr * r.wd;
    a.beta1 = beta1; a.beta2 = beta2; a.one_m_beta1 = 1.0 - beta1; a.one_m_beta2 = 1.0 - beta2; a.eps = eps;
    const float bc1 = (float)(1.0 - powi(beta1, t));
    a.bc2_sqrt = (float)sqrt(1.0 - powi(beta2, t));
    a.step_size = (float)(r.lr / (double)bc1);
    if (aligned16(r.p) && aligned16(r.g)) adamw_chunk<CLIP, true>(r, e0, m_all, v_all, a);     // (the moments: checked by the host)
    else adamw_chunk<CLIP, false>(r, e0, m_all, v_all, a);
}

static int check_table(const char* what, const void* rows, int n_rows, int64_t total_blocks) {
    if (rows == nullptr || n_rows < 0 || total_blocks < 0 || total_blocks > 0x7fffffff || (n_rows == 0 && total_blocks != 0)) {
        set_error("%s: bad table (rows %p, n_rows %d, total_blocks %lld)", what, rows, n_rows, (long long)total_blocks);
        return U3D_EINVAL;
    }
    return U3D_OK;
}

}  // namespace u3d

using namespace u3d;

extern "C" {

int u3d_optim_chunk(void) { return CHUNK; }

int64_t u3d_optim_ws_bytes(void) { return (int64_t)NPART * sizeof(double); }

int u3d_optim_grad_sumsq(const void* rows, int n_rows, int64_t total_blocks, void* ws, u3d_stream_t stream) {
    if (int rc = check_table("optim_grad_sumsq", rows, n_rows, total_blocks)) return rc;
    if (ws == nullptr || (reinterpret_cast<uintptr_t>(ws) & 7)) {
        set_error("optim_grad_sumsq: ws must be an 8-byte aligned buffer of u3d_optim_ws_bytes()");
        return U3D_EINVAL;
    }
    hipLaunchKernelGGL(optim_sumsq_k, dim3(NPART), dim3(THREADS), 0, (hipStream_t)stream, (const OptimRow*)rows, n_rows, total_blocks,
                       (double*)ws);
    return check_launch("optim_grad_sumsq");
}

int u3d_optim_adamw(const void* rows, int n_rows, int64_t total_blocks, float* exp_avg, float* exp_avg_sq, double beta1, double beta2,
                    double eps, float max_norm, int64_t step, const void* ws, float* total_norm, u3d_stream_t stream) {
    if (int rc = check_table("optim_adamw", rows, n_rows, total_blocks)) return rc;
    if (exp_avg == nullptr || exp_avg_sq == nullptr || ((reinterpret_cast<uintptr_t>(exp_avg) | reinterpret_cast<uintptr_t>(exp_avg_sq)) & 15)) {
        set_error("optim_adamw: the moment buffers must be 16-byte aligned (exp_avg %p, exp_avg_sq %p)", (void*)exp_avg, (void*)exp_avg_sq);
        return U3D_EINVAL;
    }
    const bool clip = max_norm > 0.f;
    if (step < 1 || (clip && (ws == nullptr || total_norm == nullptr || (reinterpret_cast<uintptr_t>(ws) & 7)))) {
        set_error("optim_adamw: step %lld < 1, or clipping without ws / total_norm", (long long)step);
        return U3D_EINVAL;
    }
    if (total_blocks == 0) return U3D_OK;
    if (clip)
        hipLaunchKernelGGL(optim_adamw_k<true>, dim3((unsigned)total_blocks), dim3(THREADS), 0, (hipStream_t)stream, (const OptimRow*)rows,
                           n_rows, exp_avg, exp_avg_sq, beta1, beta2, eps, max_norm, step, (const double*)ws, total_norm);
    else
        hipLaunchKernelGGL(optim_adamw_k<false>, dim3((unsigned)total_blocks), dim3(THREADS), 0, (hipStream_t)stream, (const OptimRow*)rows,
                           n_rows, exp_avg, exp_avg_sq, beta1, beta2, eps, max_norm, step, (const double*)nullptr, total_norm);
    return check_launch("optim_adamw");
}

}  // extern "C"
