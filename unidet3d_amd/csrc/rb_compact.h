// The shared pieces of the two-pass stable compaction (per-block counts -> scan of the block counts -> wave-64 ballot prefix inside each
// block): ONE definition for the pair-list builders (rulebook.hip) and the mask compaction (sparse_sets.hip).  Not part of the C ABI.
#pragma once
#include "u3d_common.h"

namespace u3d {

constexpr int RB_T = 256;

// one block per list: exclusive scan of its block counts; counts[k] = the list's total
static __global__ __launch_bounds__(RB_T) void rb_scan_k(const int32_t* __restrict__ block_cnt, int nblk, int32_t* block_base, int32_t* counts) {
    __shared__ int s_w[RB_T / 64];
    __shared__ int s_carry;
    const int k = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (int base = 0; base < nblk; base += RB_T) {
        const int i = base + threadIdx.x;
        const int v = i < nblk ? block_cnt[(int64_t)k * nblk + i] : 0;
        int incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            int t = __shfl_up(incl, d, 64);
            if (lane >= d) incl += t;
        }
        if (lane == 63) s_w[wave] = incl;
        __syncthreads();
        int woff = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < RB_T / 64; ++w) { int t = s_w[w]; if (w < wave) woff += t; tot += t; }
        const int carry = s_carry;
        if (i < nblk) block_base[(int64_t)k * nblk + i] = carry + woff + incl - v;
        __syncthreads();
        if (threadIdx.x == 0) s_carry = carry + tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) counts[k] = s_carry;
}

// position of this thread's element among the `ok` elements of its block (threads in order), for every thread of an RB_T block: the
// wave-64 ballot prefix plus the totals of the waves before it.  s_w: RB_T / 64 ints of LDS.  Every thread of the block must call it.
__device__ __forceinline__ int rb_block_rank(bool ok, int* s_w) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(ok);
    const int rank = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_w[wave] = __popcll(m);
    __syncthreads();
    int woff = 0;
#pragma unroll
    for (int w = 0; w < RB_T / 64; ++w) if (w < wave) woff += s_w[w];
    return woff + rank;
}

}  // namespace u3d
