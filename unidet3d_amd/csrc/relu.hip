// Stand-alone ReLU of a sparse layer stack (an nn.ReLU that no batch norm precedes; include/u3d.h section A1): elementwise over a flat
// fp32 buffer of ANY length -- every row count and every channel count a layer can produce.  Not on the hot path (the backbone's ReLUs
// are fused into the batch-norm kernels): one streaming pass each way, 16-byte moves where the buffers allow them, a scalar tail.
//   forward:  y[i]  = x[i] > 0 ? x[i]  : +0.0   (-0.0 and NaN give +0.0: the bits fmaxf(x * 1 + 0, 0) gave through u3d_bn_apply)
//   backward: dx[i] = x[i] > 0 ? dy[i] : +0.0   (the bits of dy where the unit is on: no arithmetic)
#include "u3d_common.h"

namespace u3d {

constexpr int RELU_T = 256;

__device__ __forceinline__ float relu_pick(float x, float v) { return x > 0.f ? v : 0.f; }

// n4 16-byte pieces, then the elements [4 n4, count); dy == nullptr: the forward (the value picked is x itself)
__global__ __launch_bounds__(RELU_T) void relu_k(const float* __restrict__ x, const float* __restrict__ dy, int64_t count, int64_t n4,
                                                 float* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * RELU_T;
    const int64_t t = (int64_t)blockIdx.x * RELU_T + threadIdx.x;
    for (int64_t i = t; i < n4; i += stride) {
        const float4 a = reinterpret_cast<const float4*>(x)[i];
        const float4 v = dy ? reinterpret_cast<const float4*>(dy)[i] : a;
        reinterpret_cast<float4*>(out)[i] = make_float4(relu_pick(a.x, v.x), relu_pick(a.y, v.y), relu_pick(a.z, v.z), relu_pick(a.w, v.w));
    }
    for (int64_t i = 4 * n4 + t; i < count; i += stride) out[i] = relu_pick(x[i], dy ? dy[i] : x[i]);
}

static int relu_launch(const char* what, const float* x, const float* dy, int64_t count, float* out, u3d_stream_t stream) {
    if (!x || !out || count <= 0) { set_error("%s: NULL pointer or no elements (count = %lld)", what, (long long)count); return U3D_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(U3D_K_BN, s, 0.0);           // an activation: booked with the norm kernels that carry every other ReLU
    const bool aligned = (((uintptr_t)x | (uintptr_t)out | (uintptr_t)dy) & 15) == 0;
    const int64_t n4 = aligned ? count / 4 : 0;
    int64_t grid = ceil_div(n4 > 0 ? n4 : count, (int64_t)RELU_T);
    if (grid > 4096) grid = 4096;               // the rest comes round the grid stride
    hipLaunchKernelGGL(relu_k, dim3((unsigned)grid), dim3(RELU_T), 0, s, x, dy, count, n4, out);
    return check_launch(what);
}

}  // namespace u3d

using namespace u3d;

extern "C" {

int u3d_relu_fwd(const float* x, int64_t count, float* y, u3d_stream_t stream) { return relu_launch("relu_fwd", x, nullptr, count, y, stream); }

int u3d_relu_bwd(const float* x, const float* dy, int64_t count, float* dx, u3d_stream_t stream) {
    if (!dy) { set_error("relu_bwd: NULL pointer"); return U3D_EINVAL; }
    return relu_launch("relu_bwd", x, dy, count, dx, stream);
}

}  // extern "C"
