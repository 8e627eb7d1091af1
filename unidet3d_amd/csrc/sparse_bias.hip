// Bias of the sparse convolution layers (bias=True; include/u3d.h section B1): y += b over every row of a convolution's fresh result,
// and db = column sums of dy.  Both are streaming passes over fp32 [n, C] with C in {32, 64, ..., 512} (the convolution's destination
// widths): a lane owns ONE 16-byte column slice for its whole life, so the bias slice (forward) and the fp64 accumulators (gradient)
// stay in registers, and rows are walked with four independent 16-byte loads in flight.
//   forward:  one fp32 addition per element, in place; rows strided over the grid; no LDS.
//   gradient: two passes, no atomics, ONE summation order (bit-identical from run to run):
//     1. workgroup b sums the FIXED row range [b R, (b + 1) R), R = U3D_BIAS_GRAD_ROWS, with fp64 accumulators (a lane adds its rows in
//        ascending order, the row slots of a workgroup are then added in slot order through LDS) and writes one fp64 row of C partials;
//     2. one wave per channel: lane l adds the partials l, l + S, l + 2 S, ... (S = U3D_BIAS_GRAD_STEP = 64) in ascending order, a fixed
//        shuffle tree adds the 64 lanes, and the fp64 sum is rounded ONCE to fp32.
// The row walk is bn_reduce_k's shape (bn.hip) but not its code: that kernel strides rows over the whole grid (its partial of a
// workgroup depends on the grid size) and carries the second sum and the backward's operands; a fixed range per workgroup is what makes
// the partial count a function of n alone here.
#include "u3d_common.h"

// every sum of this file rounds on its own, whatever the command line says (there is no product to contract today; said here so that
// it stays true)
#pragma clang fp contract(off)

namespace u3d {

constexpr int BIAS_T = 256;
constexpr int BIAS_ROWS_IN_FLIGHT = 4;

// lanes per row = C / 4 (8 .. 128), row slots per workgroup = 256 / lanes (threads past slots * lanes idle)
__global__ __launch_bounds__(BIAS_T) void bias_add_k(float* __restrict__ y, const float* __restrict__ bias, int64_t n, int C) {
    const int lpr = C >> 2, rpb = BIAS_T / lpr;
    const int c4 = threadIdx.x % lpr, slot = threadIdx.x / lpr;
    if (slot >= rpb) return;
    const float4 b = *reinterpret_cast<const float4*>(bias + c4 * 4);
    const int64_t stride = (int64_t)gridDim.x * rpb;
    for (int64_t r0 = (int64_t)blockIdx.x * rpb + slot; r0 < n; r0 += BIAS_ROWS_IN_FLIGHT * stride) {
        float4 v[BIAS_ROWS_IN_FLIGHT];
#pragma unroll
        for (int u = 0; u < BIAS_ROWS_IN_FLIGHT; ++u) {
            const int64_t r = r0 + u * stride;
            if (r < n) v[u] = *reinterpret_cast<const float4*>(y + r * C + c4 * 4);
        }
#pragma unroll
        for (int u = 0; u < BIAS_ROWS_IN_FLIGHT; ++u) {
            const int64_t r = r0 + u * stride;
            if (r < n) *reinterpret_cast<float4*>(y + r * C + c4 * 4) = make_float4(v[u].x + b.x, v[u].y + b.y, v[u].z + b.z, v[u].w + b.w);
        }
    }
}

// first pass: workgroup b owns rows [b R, min(n, (b + 1) R)); partial[b][c] = their fp64 column sum
__global__ __launch_bounds__(BIAS_T) void bias_grad_partial_k(const float* __restrict__ dy, int64_t n, int C, double* __restrict__ partial) {
    __shared__ double sh[BIAS_T * 4];
    const int lpr = C >> 2, rpb = BIAS_T / lpr;
    const int tid = threadIdx.x;
    const int c4 = tid % lpr, slot = tid / lpr;
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    if (slot < rpb) {
        const int64_t lo = (int64_t)blockIdx.x * U3D_BIAS_GRAD_ROWS;
        const int64_t hi = lo + U3D_BIAS_GRAD_ROWS < n ? lo + U3D_BIAS_GRAD_ROWS : n;
        for (int64_t r0 = lo + slot; r0 < hi; r0 += (int64_t)BIAS_ROWS_IN_FLIGHT * rpb) {
            float4 v[BIAS_ROWS_IN_FLIGHT];
#pragma unroll
            for (int u = 0; u < BIAS_ROWS_IN_FLIGHT; ++u) {
                const int64_t r = r0 + (int64_t)u * rpb;
                v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (r < hi) v[u] = *reinterpret_cast<const float4*>(dy + r * C + c4 * 4);
            }
            // rows past the end contribute exact zeros
#pragma unroll
            for (int u = 0; u < BIAS_ROWS_IN_FLIGHT; ++u) { a[0] += v[u].x; a[1] += v[u].y; a[2] += v[u].z; a[3] += v[u].w; }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) sh[tid * 4 + j] = a[j];
    __syncthreads();
    if (tid < lpr) {
        double t[4] = {0.0, 0.0, 0.0, 0.0};
        for (int s = 0; s < rpb; ++s) {
#pragma unroll
            for (int j = 0; j < 4; ++j) t[j] += sh[(s * lpr + tid) * 4 + j];
        }
        double* out = partial + (int64_t)blockIdx.x * C + tid * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) out[j] = t[j];
    }
}

// second pass: wave w of the grid owns channel w; lanes over the partial rows in steps of U3D_BIAS_GRAD_STEP, fixed shuffle tree
__global__ __launch_bounds__(BIAS_T) void bias_grad_sum_k(const double* __restrict__ partial, int64_t nblk, int C, float* __restrict__ db) {
    const int lane = threadIdx.x & 63;
    const int c = blockIdx.x * (BIAS_T / 64) + (threadIdx.x >> 6);
    if (c >= C) return;
    double t = 0.0;
    for (int64_t b = lane; b < nblk; b += U3D_BIAS_GRAD_STEP) t += partial[b * C + c];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) t += __shfl_xor(t, d, 64);
    if (lane == 0) db[c] = (float)t;
}

// the contract both entry points share, checked before any HIP call
static int check_bias(const char* what, const void* a, const void* b, int64_t n, int C) {
    if (!a || !b || n <= 0) { set_error("%s: NULL pointer or no rows (n = %lld)", what, (long long)n); return U3D_EINVAL; }
    if (C < 32 || C > 512 || C % 32) { set_error("%s: width %d unsupported (a multiple of 32 in 32..512, the convolution's destination widths)", what, C); return U3D_EUNSUPPORTED; }
    if (n > 0x7fffffffLL) { set_error("%s: %lld rows exceed 32-bit row counts", what, (long long)n); return U3D_EUNSUPPORTED; }
    return U3D_OK;
}

static_assert(U3D_BIAS_GRAD_STEP == 64, "bias_grad_sum_k: one wave per channel, one partial per lane and step");

}  // namespace u3d

using namespace u3d;

extern "C" {

int u3d_bias_add(float* y, const float* bias, int64_t n, int C, u3d_stream_t stream) {
    const int rc = check_bias("bias_add", y, bias, n, C);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(U3D_K_CONV_FWD, s, 0.0);      // the tail of a convolution layer's forward: booked with it
    const int rpb = BIAS_T / (C >> 2);
    int64_t grid = ceil_div(n, (int64_t)rpb * BIAS_ROWS_IN_FLIGHT);
    if (grid > 2048) grid = 2048;           // 8 workgroups per CU: the rest of the rows come round the grid stride
    hipLaunchKernelGGL(bias_add_k, dim3((unsigned)grid), dim3(BIAS_T), 0, s, y, bias, n, C);
    return check_launch("bias_add");
}

int64_t u3d_bias_grad_ws_bytes(int64_t n, int C) {
    if (n <= 0 || C <= 0) return 0;
    return ceil_div(n, U3D_BIAS_GRAD_ROWS) * C * (int64_t)sizeof(double);
}

int u3d_bias_grad(const float* dy, int64_t n, int C, float* db, void* ws, u3d_stream_t stream) {
    const int rc = check_bias("bias_grad", dy, db, n, C);
    if (rc) return rc;
    if (!ws) { set_error("bias_grad: NULL workspace (u3d_bias_grad_ws_bytes)"); return U3D_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(U3D_K_CONV_WGRAD, s, 0.0);    // a convolution layer's parameter gradient: booked with its weight gradient
    const int64_t nblk = ceil_div(n, U3D_BIAS_GRAD_ROWS);
    hipLaunchKernelGGL(bias_grad_partial_k, dim3((unsigned)nblk), dim3(BIAS_T), 0, s, dy, n, C, (double*)ws);
    hipLaunchKernelGGL(bias_grad_sum_k, dim3((unsigned)ceil_div(C, BIAS_T / 64)), dim3(BIAS_T), 0, s, (const double*)ws, nblk, C, db);
    return check_launch("bias_grad");
}

}  // extern "C"
