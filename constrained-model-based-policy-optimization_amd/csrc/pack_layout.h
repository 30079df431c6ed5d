// The packed-weight layouts of the MFMA kernels: the only place that knows them (not part of the public ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

// fp32 pack of a [K][N] matrix, [n-tile 32][k-group 8][lane 64][4]: a lane's float4 is the fragment of four
// v_mfma_f32_32x32x2f32 (column n & 31 of the tile, k = 8 g + 4 (lane >> 5) + 0..3).
// float index within a member of element k of column r (< 32) of n-tile `tile`
__host__ __device__ __forceinline__ constexpr size_t pack_index_tile(int tile, int r, int k, int kg) {
  return (((size_t)tile * kg + (k >> 3)) * 64 + ((k >> 2) & 1) * 32 + r) * 4 + (k & 3);
}
__host__ __device__ __forceinline__ constexpr size_t pack_index(int k, int n, int kg) { return pack_index_tile(n >> 5, n & 31, k, kg); }
// the inverse map: float index -> (k, n)
__host__ __device__ __forceinline__ void pack_unindex(int i, int kg, int &k, int &n) {
  const int s = i & 3, lane = (i >> 2) & 63, g = (i >> 8) % kg, nt = (i >> 8) / kg;
  n = nt * 32 + (lane & 31);
  k = 8 * g + 4 * (lane >> 5) + s;
}
// floats per member
__host__ __device__ __forceinline__ constexpr size_t pack_floats(int n_tiles, int kg) { return (size_t)n_tiles * kg * 256; }

// Strides and offsets that kernels compute on their hot paths are macros: the products then compile exactly as if spelled
// out in place (as an inlined function the same arithmetic reaches the optimiser in another order, and ens_mlp_kernel<512>
// comes out with other registers).
// the pack in float4 units (a lane's fragment of one k-group): n_tiles tiles of kg k-groups
#define PACK_VEC4S(n_tiles, kg) ((size_t)(n_tiles) * (kg) * 64)

// f16 / bf16 images [n-tile 32][k-slab 16][piece][lane 64] of 8 halves (2 pieces: f16_split.h, 3: ens_split.hip), 16-byte units:
// the lanes of one piece, n_tiles tiles of `slabs` slabs (a member's size), and the first lane's fragment (tile, slab, piece)
constexpr int kImageLanes = 64;
#define IMAGE_UNITS(n_tiles, slabs, pieces) ((size_t)(n_tiles) * (slabs) * (pieces) * kImageLanes)
#define IMAGE_INDEX(tile, slabs, slab, pieces, piece) (((size_t)((tile) * (slabs) + (slab)) * (pieces) + (piece)) * kImageLanes)
