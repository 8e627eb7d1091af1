// The dropout mask of the decoder: a stateless hash of (seed, offset, a, b, c) to 32 bits, ONE definition for the
// attention kernels (a, b, c = head, packed query row, packed key row), the elementwise kernels (0, row, column) and the two mask
// dumps.  No mask is stored anywhere: forward and backward call the same function with the same arguments.
//
//     keep(seed, offset, a, b, c)  <=>  drop_hash32(...) >= thr,     thr = floor(p 2^32), computed on the host in double
//
// The function is staged by how often its arguments change, so that a kernel pays per element only for what varies per element:
//   drop_key(seed, offset, a)   64 bits (k0, k1): three splitmix64 finalisers over the wave-uniform arguments -- scalar ALU, once per kernel
//   drop_row(key, b)            64 bits (x, y):   x = (b + k0) M1, x ^= x >> 16;  y = b M2 + k1.  Once per lane where a lane owns a row b
//                                                 (forward, dQ); where b runs over four consecutive rows (dK / dV) b M1 and b M2 advance by
//                                                 adding a constant, and the xor-shift is the per-element cost
//   drop_hash32(row, c)         h = (x + c) M3;  h ^= h >> 15;  h = (h + y) M4          two multiply / xor-shift rounds over c
// c enters by addition, so consecutive c (a lane's four keys, a thread's eight columns) cost one add of a literal each.  Two rows whose
// x differ by less than the row length would hold shifted copies of one mask after the first round; y, an independent 32 bits of the
// row, is what the second round adds, so they do not.  The last product is compared as it is: the comparison with thr reads the high
// bits, which a multiply mixes best.  tests/_dropout.py restates the function in numpy; tests/test_gpu_dropout.py pins the two together.
#pragma once
#include <stdint.h>

namespace u3d {

struct DropKey { uint32_t k0, k1; };
struct DropRow { uint32_t x, y; };

constexpr uint32_t DROP_M1 = 0x9E3779B1u, DROP_M2 = 0x85EBCA77u, DROP_M3 = 0xCC9E2D51u, DROP_M4 = 0x1B873593u;

__host__ __device__ inline uint64_t drop_mix64(uint64_t z) {          // splitmix64
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__host__ __device__ inline DropKey drop_key(uint64_t seed, uint64_t offset, uint32_t a) {
    const uint64_t z = drop_mix64(drop_mix64(drop_mix64(seed) ^ offset) ^ (uint64_t)a);
    return DropKey{(uint32_t)z, (uint32_t)(z >> 32)};
}
__host__ __device__ inline DropRow drop_row(DropKey k, uint32_t b) {
    uint32_t x = (b + k.k0) * DROP_M1;
    x ^= x >> 16;
    return DropRow{x, b * DROP_M2 + k.k1};
}
__host__ __device__ inline uint32_t drop_hash32(DropRow r, uint32_t c) {
    uint32_t h = (r.x + c) * DROP_M3;
    h ^= h >> 15;
    return (h + r.y) * DROP_M4;
}
__host__ __device__ inline bool drop_keep(uint64_t seed, uint64_t offset, uint32_t a, uint32_t b, uint32_t c, uint32_t thr) {
    return drop_hash32(drop_row(drop_key(seed, offset, a), b), c) >= thr;
}

// what a kernel receives: the key of the call, the threshold and 1 / (1 - p) rounded once to fp32
struct DropArgs {
    uint64_t seed, offset;
    uint32_t thr;
    float rinv;
};
// host: p in [0, 1) (validated by the caller) -> (thr, rinv)
inline DropArgs drop_args(double p, uint64_t seed, uint64_t offset) {
    return DropArgs{seed, offset, (uint32_t)(p * 4294967296.0), (float)(1.0 / (1.0 - p))};
}

}  // namespace u3d
