// Dense interchange of sparse tensors (include/u3d.h section S2): rows -> dense grid (`SparseConvTensor.dense`), dense grid -> rows at
// given coordinates (its backward), the activity mask of a channels-last grid and the coordinates of cell numbers (`from_dense`).
// Every kernel is a copy: bits travel untouched, every destination element is written exactly once, no atomics, no memset.
// Dense cell number of (b, x, y, z) = ((b X + x) Y + y) Z + z < 2^31 (NOT the occupancy index's cell id, which pads z lines to whole
// bitmap words); element offsets are 64-bit (cells x C passes 2^31 on real BEV grids).
// Channels last [B, X, Y, Z, C]: the lane shape of sparse_sets.hip's rows_take_k -- a group of 2^lg lanes owns a destination cell / row
// and 16-byte column slices, CELLS of them in flight, a column loop past 256 channels.
// Channels first [B, C, X, Y, Z]: a transpose through LDS.  A workgroup owns 64 consecutive cell numbers of ONE batch item (scatter) or
// 64 consecutive rows (gather) x a chunk of 64 channels; the tile's row stride is 65 dwords, odd against the 64 banks, so both the
// row-wise and the channel-wise walk of it are conflict free.  The plane stride X Y Z is arbitrary: the dense side moves dwords, one per
// lane, 256-byte runs per channel; the row side moves 16-byte slices.  16.6 KB of LDS per workgroup: nine workgroups per CU.
#include "u3d_common.h"

namespace u3d {

constexpr int CELLS = 4;            // destination cells / rows of one lane group in flight (channels last)
constexpr int TILE = 64;            // cells / rows of a channels-first tile: one lane each
constexpr int CHUNK = 64;           // channels of a channels-first tile
constexpr int LDW = CHUNK + 1;      // its LDS row stride in dwords

// (b, x, y, z) of a dense cell number
__device__ __forceinline__ int4 cell_coords(unsigned cell, int X, int Y, int Z) {
    const unsigned z = cell % (unsigned)Z, t = cell / (unsigned)Z, y = t % (unsigned)Y, u = t / (unsigned)Y;
    return make_int4((int)(u / (unsigned)X), (int)(u % (unsigned)X), (int)y, (int)z);
}

// dense cell number of a coordinate row, -1 outside the grid or the batch (unsigned compares: negative components are outside)
__device__ __forceinline__ int64_t cell_of(const int4 c, int B, int X, int Y, int Z) {
    if ((unsigned)c.x >= (unsigned)B || (unsigned)c.y >= (unsigned)X || (unsigned)c.z >= (unsigned)Y || (unsigned)c.w >= (unsigned)Z) return -1;
    return (((int64_t)c.x * X + c.y) * Y + c.z) * Z + c.w;
}

// ---- channels last ------------------------------------------------------------------------------------------------------------------
// group g serves the cells g, g + G, ...; lane l of it the columns 4 l + (4 << lg) i.  A looked-up row outside [0, n) is an absent row.
__global__ __launch_bounds__(256) void scatter_last_k(const uint4* __restrict__ x, int64_t n, Index ix, int64_t n_cells, int64_t G, int C4,
                                                      int lg, uint4* __restrict__ y) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t g = t >> lg;
    const int c0 = (int)(t & ((1 << lg) - 1));
    if (g >= G) return;
    int r[CELLS];
#pragma unroll
    for (int u = 0; u < CELLS; ++u) {
        r[u] = -1;
        if (g + u * G < n_cells) {
            const int4 c = cell_coords((unsigned)(g + u * G), ix.X, ix.Y, ix.Z);
            r[u] = index_lookup(ix, c.x, c.y, c.z, c.w);
        }
    }
    for (int c = c0; c < C4; c += 1 << lg) {
        uint4 v[CELLS];
#pragma unroll
        for (int u = 0; u < CELLS; ++u) {
            v[u] = make_uint4(0u, 0u, 0u, 0u);
            if ((uint64_t)(int64_t)r[u] < (uint64_t)n) v[u] = x[(int64_t)r[u] * C4 + c];
        }
#pragma unroll
        for (int u = 0; u < CELLS; ++u)
            if (g + u * G < n_cells) y[(g + u * G) * C4 + c] = v[u];
    }
}

// group g serves the rows g, g + G, ...: a row copy from a computed address
__global__ __launch_bounds__(256) void gather_last_k(const uint4* __restrict__ dense, int B, int X, int Y, int Z, const int4* __restrict__ coords,
                                                     int64_t n, int64_t G, int C4, int lg, uint4* __restrict__ rows) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t g = t >> lg;
    const int c0 = (int)(t & ((1 << lg) - 1));
    if (g >= G) return;
    int64_t cell[CELLS];
#pragma unroll
    for (int u = 0; u < CELLS; ++u) cell[u] = g + u * G < n ? cell_of(coords[g + u * G], B, X, Y, Z) : -1;
    for (int c = c0; c < C4; c += 1 << lg) {
        uint4 v[CELLS];
#pragma unroll
        for (int u = 0; u < CELLS; ++u) {
            v[u] = make_uint4(0u, 0u, 0u, 0u);
            if (cell[u] >= 0) v[u] = dense[cell[u] * C4 + c];
        }
#pragma unroll
        for (int u = 0; u < CELLS; ++u)
            if (g + u * G < n) rows[(g + u * G) * C4 + c] = v[u];
    }
}

// ---- channels first -----------------------------------------------------------------------------------------------------------------
// the 16-byte slices of a tile: slice j = threadIdx.x + 256 u -> tile row j / 16, columns 4 (j % 16) .. + 3
constexpr int SLICES = TILE * (CHUNK / 4) / 256;

// block = (batch item, tile of 64 cell numbers inside it, channel chunk), the chunk running fastest
__global__ __launch_bounds__(256) void scatter_first_k(const uint4* __restrict__ x, int64_t n, Index ix, int64_t S, unsigned tiles, unsigned chunks,
                                                       int C, uint32_t* __restrict__ y) {
    __shared__ uint32_t s_t[TILE * LDW];
    __shared__ int s_row[TILE];
    const unsigned ch = blockIdx.x % chunks, bt = blockIdx.x / chunks;
    const int b = (int)(bt / tiles);
    const int64_t s0 = (int64_t)(bt % tiles) * TILE;
    const int c0 = (int)ch * CHUNK;
    const int cw = min(CHUNK, C - c0);
    if (threadIdx.x < TILE) {
        const int64_t s = s0 + threadIdx.x;
        int r = -1;
        if (s < S) {
            const int4 c = cell_coords((unsigned)s, ix.X, ix.Y, ix.Z);      // (batch item 0: s < S)
            r = index_lookup(ix, b, c.y, c.z, c.w);
        }
        s_row[threadIdx.x] = r;
    }
    __syncthreads();
    uint4 v[SLICES];
#pragma unroll
    for (int u = 0; u < SLICES; ++u) {
        const int j = threadIdx.x + 256 * u, q = j & 15;
        const int r = s_row[j >> 4];
        v[u] = make_uint4(0u, 0u, 0u, 0u);
        if (4 * q < cw && (uint64_t)(int64_t)r < (uint64_t)n) v[u] = x[(int64_t)r * (C / 4) + c0 / 4 + q];
    }
#pragma unroll
    for (int u = 0; u < SLICES; ++u) {
        const int j = threadIdx.x + 256 * u;
        uint32_t* d = s_t + (j >> 4) * LDW + 4 * (j & 15);
        d[0] = v[u].x; d[1] = v[u].y; d[2] = v[u].z; d[3] = v[u].w;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (s0 + lane >= S) return;
    uint32_t* out = y + ((int64_t)b * C + c0) * S + s0 + lane;
    for (int k = w; k < cw; k += 4) out[(int64_t)k * S] = s_t[lane * LDW + k];
}

// block = (tile of 64 consecutive rows, channel chunk); lane = row on the dense side
__global__ __launch_bounds__(256) void gather_first_k(const uint32_t* __restrict__ dense, int B, int X, int Y, int Z, int64_t S,
                                                      const int4* __restrict__ coords, int64_t n, unsigned chunks, int C, uint4* __restrict__ rows) {
    __shared__ uint32_t s_t[TILE * LDW];
    const unsigned ch = blockIdx.x % chunks;
    const int64_t r0 = (int64_t)(blockIdx.x / chunks) * TILE;
    const int c0 = (int)ch * CHUNK;
    const int cw = min(CHUNK, C - c0);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int64_t base = -1;
    if (r0 + lane < n) {
        const int4 c = coords[r0 + lane];
        const int64_t cell = cell_of(c, B, X, Y, Z);
        if (cell >= 0) base = ((int64_t)c.x * C + c0) * S + (cell - (int64_t)c.x * S);
    }
    for (int k = w; k < cw; k += 4) s_t[lane * LDW + k] = base >= 0 ? dense[base + (int64_t)k * S] : 0u;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < SLICES; ++u) {
        const int j = threadIdx.x + 256 * u, q = j & 15;
        const int64_t r = r0 + (j >> 4);
        if (4 * q >= cw || r >= n) continue;
        const uint32_t* d = s_t + (j >> 4) * LDW + 4 * q;
        rows[r * (C / 4) + c0 / 4 + q] = make_uint4(d[0], d[1], d[2], d[3]);
    }
}

// ---- from_dense's geometry ----------------------------------------------------------------------------------------------------------
// mask[cell] = any of the cell's C values != 0 (a NaN compares unequal: active; -0.0 compares equal: not).  The group's lanes OR their
// slices, one ballot per cell in flight reduces the group, its first lane writes the byte.  No thread leaves before the ballots.
__global__ __launch_bounds__(256) void dense_active_k(const float4* __restrict__ x, int64_t n_cells, int64_t G, int C4, int lg,
                                                      uint8_t* __restrict__ mask) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t g = t >> lg;
    const int gs = 1 << lg, c0 = (int)(t & (gs - 1)), lane = threadIdx.x & 63;
    bool any[CELLS];
#pragma unroll
    for (int u = 0; u < CELLS; ++u) any[u] = false;
    for (int c = c0; c < C4; c += gs) {
        float4 v[CELLS];
#pragma unroll
        for (int u = 0; u < CELLS; ++u) {
            v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (g < G && g + u * G < n_cells) v[u] = x[(g + u * G) * C4 + c];
        }
#pragma unroll
        for (int u = 0; u < CELLS; ++u) any[u] |= v[u].x != 0.f || v[u].y != 0.f || v[u].z != 0.f || v[u].w != 0.f;
    }
    const uint64_t mine = (gs == 64 ? ~0ull : (1ull << gs) - 1ull) << (lane & ~(gs - 1));
#pragma unroll
    for (int u = 0; u < CELLS; ++u) {
        const uint64_t m = __ballot(any[u]);
        if (c0 == 0 && g < G && g + u * G < n_cells) mask[g + u * G] = (m & mine) != 0 ? 1 : 0;
    }
}

// thread = row, one 16-byte store
__global__ __launch_bounds__(256) void cells_coords_k(const int32_t* __restrict__ cells, int64_t n, int X, int Y, int Z, int4* __restrict__ coords) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) coords[i] = cell_coords((unsigned)cells[i], X, Y, Z);
}

// lanes per cell / row: the power of two that covers C / 4, one wave at most (sparse_sets.hip's rule)
static int lanes_log2(int C) {
    int lg = 0;
    while (lg < 6 && (4 << lg) < C) ++lg;
    return lg;
}

// ---- the contract, checked before any HIP call ----------------------------------------------------------------------------------------
static int check_width(const char* what, int C) {
    if (C < 4 || C > 512 || C % 4) { set_error("%s: width %d unsupported (a multiple of 4 in 4..512)", what, C); return U3D_EUNSUPPORTED; }
    return U3D_OK;
}

// B X Y Z cells, every factor positive, the product below 2^31 (32-bit cell numbers); the running product stays below 2^62
static int check_grid(const char* what, int B, int X, int Y, int Z, int64_t* cells) {
    if (B <= 0 || X <= 0 || Y <= 0 || Z <= 0) { set_error("%s: an empty grid %d x %d x %d x %d", what, B, X, Y, Z); return U3D_EINVAL; }
    int64_t c = B;
    const int dims[3] = {X, Y, Z};
    for (int d : dims) {
        c *= d;
        if (c >= 0x80000000LL) {
            set_error("%s: the grid %d x %d x %d x %d has 2^31 cells or more: cell numbers are 32-bit", what, B, X, Y, Z);
            return U3D_EUNSUPPORTED;
        }
    }
    *cells = c;
    return U3D_OK;
}

// one 256-thread block per unit of work on a one-dimensional grid: the launch takes fewer than 2^32 threads
static int check_blocks(const char* what, int64_t blocks) {
    if (blocks >= (1LL << 24)) { set_error("%s: %lld workgroups exceed one launch (2^24 of 256 threads)", what, (long long)blocks); return U3D_EUNSUPPORTED; }
    return U3D_OK;
}

static int check_rows(const char* what, bool null, int64_t n) {
    if (null || n <= 0) { set_error("%s: NULL pointer or no rows (n = %lld)", what, (long long)n); return U3D_EINVAL; }
    if (n >= 0x80000000LL) { set_error("%s: %lld rows exceed 32-bit row numbers", what, (long long)n); return U3D_EUNSUPPORTED; }
    return U3D_OK;
}

}  // namespace u3d

using namespace u3d;

extern "C" {

int u3d_dense_scatter(const float* feats, int64_t n, int C, const uint64_t* bitmap, const int32_t* word_rank, int64_t hash_slots, int B, int X,
                      int Y, int Z, int channels_first, float* dense, u3d_stream_t stream) {
    int rc = check_rows("dense_scatter", !feats || !bitmap || !word_rank || !dense, n);
    if (rc) return rc;
    if (hash_slots < 0) { set_error("dense_scatter: negative hash_slots"); return U3D_EINVAL; }
    int64_t n_cells = 0;
    if ((rc = check_width("dense_scatter", C)) || (rc = check_grid("dense_scatter", B, X, Y, Z, &n_cells))) return rc;
    const int64_t S = n_cells / B, tiles = ceil_div(S, TILE), chunks = ceil_div(C, CHUNK);
    const int lg = lanes_log2(C);
    const int64_t G = ceil_div(n_cells, CELLS);
    const int64_t blocks = channels_first ? B * tiles * chunks : ceil_div(G << lg, 256);
    if ((rc = check_blocks("dense_scatter", blocks))) return rc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(U3D_K_POOL, s, 0.0);
    const Index ix = make_index(bitmap, word_rank, B, X, Y, Z, hash_slots);
    if (channels_first) {
        hipLaunchKernelGGL(scatter_first_k, dim3((unsigned)blocks), dim3(256), 0, s, reinterpret_cast<const uint4*>(feats), n, ix, S,
                           (unsigned)tiles, (unsigned)chunks, C, reinterpret_cast<uint32_t*>(dense));
    } else {
        hipLaunchKernelGGL(scatter_last_k, dim3((unsigned)blocks), dim3(256), 0, s, reinterpret_cast<const uint4*>(feats), n, ix,
                           n_cells, G, C / 4, lg, reinterpret_cast<uint4*>(dense));
    }
    return check_launch("dense_scatter");
}

int u3d_dense_gather(const float* dense, int B, int X, int Y, int Z, int C, int channels_first, const int32_t* coords, int64_t n, float* rows,
                     u3d_stream_t stream) {
    int rc = check_rows("dense_gather", !dense || !coords || !rows, n);
    if (rc) return rc;
    int64_t n_cells = 0;
    if ((rc = check_width("dense_gather", C)) || (rc = check_grid("dense_gather", B, X, Y, Z, &n_cells))) return rc;
    const int64_t chunks = ceil_div(C, CHUNK);
    const int lg = lanes_log2(C);
    const int64_t G = ceil_div(n, CELLS);
    const int64_t blocks = channels_first ? ceil_div(n, TILE) * chunks : ceil_div(G << lg, 256);
    if ((rc = check_blocks("dense_gather", blocks))) return rc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(U3D_K_POOL, s, 0.0);
    if (channels_first) {
        hipLaunchKernelGGL(gather_first_k, dim3((unsigned)blocks), dim3(256), 0, s, reinterpret_cast<const uint32_t*>(dense), B, X,
                           Y, Z, n_cells / B, reinterpret_cast<const int4*>(coords), n, (unsigned)chunks, C, reinterpret_cast<uint4*>(rows));
    } else {
        hipLaunchKernelGGL(gather_last_k, dim3((unsigned)blocks), dim3(256), 0, s, reinterpret_cast<const uint4*>(dense), B, X, Y, Z,
                           reinterpret_cast<const int4*>(coords), n, G, C / 4, lg, reinterpret_cast<uint4*>(rows));
    }
    return check_launch("dense_gather");
}

int u3d_dense_active(const float* x, int64_t n_cells, int C, uint8_t* mask, u3d_stream_t stream) {
    int rc = check_rows("dense_active", !x || !mask, n_cells);
    if (rc || (rc = check_width("dense_active", C))) return rc;
    const int lg = lanes_log2(C);
    const int64_t G = ceil_div(n_cells, CELLS);
    if ((rc = check_blocks("dense_active", ceil_div(G << lg, 256)))) return rc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(U3D_K_RULEBOOK, s, 0.0);
    hipLaunchKernelGGL(dense_active_k, dim3((unsigned)ceil_div(G << lg, 256)), dim3(256), 0, s, reinterpret_cast<const float4*>(x), n_cells, G, C / 4,
                       lg, mask);
    return check_launch("dense_active");
}

int u3d_cells_coords(const int32_t* cells, int64_t n, int X, int Y, int Z, int32_t* coords, u3d_stream_t stream) {
    int rc = check_rows("cells_coords", !cells || !coords, n);
    if (rc) return rc;
    int64_t per_item = 0;
    if ((rc = check_grid("cells_coords", 1, X, Y, Z, &per_item))) return rc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(U3D_K_RULEBOOK, s, 0.0);
    hipLaunchKernelGGL(cells_coords_k, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, cells, n, X, Y, Z, reinterpret_cast<int4*>(coords));
    return check_launch("cells_coords");
}

}  // extern "C"
