// Ensemble forward (HEAD_PROB, 512-wide, swish) with every float32 product carried by THREE f16 MFMAs.
//
// Same function as ens_mlp_kernel<512, *, swish, prob> / ens_split_kernel (models/pens/pe.py:688-697,789-838,
// fc.py:74-95, models/pens/utils.py:156-187): one item = 128 rows of one member through
//     x -> swish(x W0 + b0) -> swish(. W1 + b1) -> . W2 + b2 -> (mean, var).
//
// Arithmetic.  A float32 number a, lifted by a power of two s into the top of the f16 range, splits into two f16
// pieces a1 = f16(a s), a2 = f16(a s - a1) (the difference is exact in float32): 11 + 1 + 11 significant bits, i.e.
// a s = (a1 + a2)(1 + d), |d| <= 2^-24 -- a float32 rounding.  Then
//     a . b  =  [a2 b1 + a1 b2 + a1 b1] / (s t)  +  O(2^-23 |ab|)
// as three f16 MFMAs with fp32 accumulation (32x32x16 in layer 0, 16x16x32 in layers 1 and 2) (every partial product exact, smallest first; the dropped
// a2 b2 <= 2^-24 |ab|).  Measured (tools/split_f16_probe.hip): error 3.2e-7 of sum|a_k b_k| at K = 512 -- the fp32 MFMA
// chain 7.6e-7, the six-term bf16 split 6.2e-7 -- at half the matrix instructions of the latter.
// Scales (all powers of two, so scaling and unscaling are exact):
//   * weights: one per (member, layer), max |W| s in [2^13, 2^14)  (h3_stats_kernel, whenever the packs change);
//   * activations: one per (row, layer), from a BOUND known before the layer runs: the row's max |x| is taken when the
//     input is staged, and |h1| <= |z1| <= L1 m0 + B, |h2| <= L2 bound1 + B' with L = the member's largest column 1-norm
//     of W and B = max |b| (swish(z) <= |z|).  bound t in [2^13, 2^14): no piece can overflow for any finite input, no
//     cross-wave reduction is needed, and a loose bound only moves the SMALLEST elements of a row towards the f16
//     subnormals: an element keeps full relative precision down to 2^-17 of the bound, below that its absolute error is
//     <= 2^-39 of the bound.  Non-finite inputs give non-finite outputs for their own row only (rows are MFMA columns).
//
// Work decomposition (what round 1's stamps asked for): 512 threads = 8 waves = two per SIMD, so the non-matrix
// phases issue VALU at the SIMD's full rate and one wave's waits hide behind its partner's MFMAs; 128-row items, so a
// weight fragment fetched from L2 feeds four 32-row tiles (the probe's slab loop is L2 -> CU bound at 64 rows: 489 ->
// 680 ns per slab with the loads); every activation is split ONCE, by the wave that produced it, into two f16 images in
// LDS which all waves read as ready MFMA operands (no VALU in the slab loop).  A 128-row h1 image would need 266 KB, so
// layers 0 and 1 are fused over k: chunk c of h1 (64 hidden units x 128 rows, 8 (n-tile, row-tile) pairs = one per
// wave) is produced into a double-buffered 36 KB image while the layer-1 MFMAs consume chunk c - 1.  Wave w owns hidden
// n-tiles 2w, 2w+1 x four row tiles of layer 1 (128 accumulator registers).  h2 leaves the accumulators in two 64-row
// halves through a [64][512] image; the output layer is split over (output tile, row tile, k half) units, its results
// pass through an LDS staging tile so that rows are stored as contiguous runs.
//
// The split input image does not depend on the member.  The main launch of 128-row items on the stage-ahead instances
// takes it ready from h3_ximage_kernel, which builds it once per row in front of that launch, instead of building it once
// per (member, row): a tile's block travels to LDS by LDS-DMA, requested behind the weight ring's last wait of the
// predecessor's last fused step (ens_h3_kernel<.., IMG = true>, piece_at_img).  Every other launch stages its
// rows itself, as before.
#include "common.h"
#include "ens_mlp_internal.h"
#include "f16_split.h"

#include <type_traits>

namespace {

constexpr int kThreadsH = 512;
constexpr int kWavesH = 8;
constexpr int HIDH = 512;

// Geometry of an item of RT 32-row tiles (4: the throughput shape; 2 / 1: the same kernel for rollout batches too small
// to give every CU a 128-row item -- an item's latency is the step's there).  Whatever RT, a chunk of h1 is 8 (n-tile,
// row-tile) pairs = one per wave, and a step of the fused layer-0/1 loop is 16 (32-deep slab, 16-row tile) positions of
// 12 v_mfma_f32_16x16x32_f16 (4 hidden 16-tiles x 3 terms).
template <int RT>
struct Geo {
  static constexpr int ROWS = 32 * RT;
  static constexpr int NTC = 8 / RT;           // hidden n-tiles per chunk
  static constexpr int CK = 32 * NTC;          // hidden units per chunk
  static constexpr int NCH = HIDH / CK;        // chunks
  static constexpr int SLC = CK / 32;          // 32-deep layer-1 slabs per chunk
  static constexpr int CSTR = CK + 8;          // row stride (halves) of a chunk image: 16-B slots per row odd -> conflict-free
  static constexpr int TPR = kThreadsH / ROWS; // threads staging one input row
  static constexpr int KPT = 64 / TPR;         // input elements per staging thread
  // ring of layer-1 weight fragments in half slabs (4 f16x8 = 16 registers: two hidden 16-tiles x two pieces): a half is
  // requested as soon as the one DH halves before it has fed its last MFMA.  At 128 rows (128 accumulator registers) two:
  // a half arrives 6 MFMAs ahead of its use (a third spills ~70 registers in the loop).
  static constexpr int DH = RT == 4 ? 2 : 4;
  static constexpr int NPH = (2 * SLC) % DH == 0 ? 1 : DH;   // steps after which the ring's registers line up again
  static constexpr int CBUF_BYTES = 2 * ROWS * CSTR * 2;          // one chunk image (both pieces)
  static constexpr bool W0_LDS = RT == 4;      // W0 fragments shared by several waves pass through LDS
};

// ---- LDS map (bytes) ---------------------------------------------------------------------------------------------
// An item after the first of a workgroup is staged AHEAD -- its split input image, per-row scales, constants and the first
// two W0 chunks are written during the last step of its predecessor's fused loop, whose tail then still runs -- so what the
// stage writes lies behind everything the tail touches, and the per-item constants exist twice (by item parity):
// [0, ...)            layers 0 / 1: chunk images [2][2 pieces][ROWS][CSTR]
//                     tail (aliases them): partial outputs [8 waves][2 tiles][16][64] f32 | staging [2][32][SWS]
// [OFF_XIMG, ...)     x image [2][ROWS][XSTR] | W0 chunk [2][4 S0 KB]
// [OFF_CONST, ...)    2 x { bias0 | bias1 | head constants | per-row scales } | input scaler
// That fits the CU's 160 KB only with ONE buffer of partial outputs (64 KB; two would put the tail alone at 147 712 B), at
// the price of a second barrier per tail unit between the sum over the previous unit's partials and the next write.
// <4, *, 4> alone keeps the old order (the stage at the top of every item, one copy of the constants, two buffers of
// partial outputs, which cover the x image and the W0 chunks): LDS forces it -- 82 176 B of tail buffers + 69 632 B of
// x image and W0 chunks + two constants copies 16 896 B = 168 704 B against the CU's 163 840.
constexpr int PBUF_BYTES = kWavesH * 2 * 16 * 64 * 4;     // partial outputs of one unit: [8 waves][2 tiles][4][64 lanes] x 16 B
constexpr int SWS = 65;                                   // row stride of a staging tile (floats): odd
constexpr int STG_BYTES = 32 * SWS * 4;
__host__ __device__ constexpr bool stage_ahead(int S0, int RT) { return !(S0 == 4 && RT == 4); }
__host__ __device__ constexpr int tail_bytes(int S0, int RT) { return (stage_ahead(S0, RT) ? 1 : 2) * PBUF_BYTES + 2 * STG_BYTES; }
__host__ __device__ constexpr int ximg_bytes(int S0, int RT) { return 2 * 32 * RT * (16 * S0 + 8) * 2; }
__host__ __device__ constexpr int w0buf_bytes(int S0, int RT) { return RT == 4 ? 2 * S0 * 2 * 1024 : 0; }   // one chunk
__host__ __device__ constexpr int r16(int v) { return (v + 15) / 16 * 16; }
__host__ __device__ constexpr int off_ximg(int S0, int RT) {
  const int cb = 2 * (RT == 4 ? Geo<4>::CBUF_BYTES : (RT == 2 ? Geo<2>::CBUF_BYTES : Geo<1>::CBUF_BYTES));
  return stage_ahead(S0, RT) && tail_bytes(S0, RT) > cb ? r16(tail_bytes(S0, RT)) : cb;
}
__host__ __device__ constexpr int off_const(int S0, int RT) {
  const int a = off_ximg(S0, RT) + ximg_bytes(S0, RT) + 2 * w0buf_bytes(S0, RT);
  return r16(a > tail_bytes(S0, RT) ? a : tail_bytes(S0, RT));
}
constexpr int ITEM_FLOATS = 2 * HIDH + 2 * 128 + 6 * 128;     // the per-item constants
__host__ __device__ constexpr int lds_bytes(int S0, int RT) {
  return off_const(S0, RT) + ((stage_ahead(S0, RT) ? 2 : 1) * ITEM_FLOATS + 2 * 64) * 4;
}
static_assert(lds_bytes(4, 4) == 156416 && lds_bytes(3, 4) == 152320 && lds_bytes(2, 4) <= 160 * 1024 &&
              lds_bytes(4, 2) <= 160 * 1024 && lds_bytes(4, 1) <= 160 * 1024, "ens_h3: LDS map");

#ifdef CMBPO_STAMPS
#define H3_STAMP(k)                                                         \
  do {                                                                      \
    __builtin_amdgcn_sched_barrier(0);                                      \
    const unsigned long long t_now = __builtin_amdgcn_s_memtime();          \
    __builtin_amdgcn_s_waitcnt(0xC07F);                                     \
    t_acc[k] += t_now - t_last;                                             \
    t_last = t_now;                                                         \
    __builtin_amdgcn_sched_barrier(0);                                      \
  } while (0)
#else
#define H3_STAMP(k) do { } while (0)
#endif

// ---- per-member statistics of the fp32 packs: max |W|, largest column 1-norm, max |b| -----------------------------------
// pack layout [n-tile][k-group][lane (r, h)][4]: W[k = 8 g + 4 h + s][n = 32 tile + r].  grid (E, 3), 512 threads.
__global__ void h3_stats_kernel(const float *blob, size_t off0, size_t off1, size_t off2, size_t offb0, size_t offb1, size_t offb2,
                                int kg0, int o_tiles, int hidden, float *stats) {
  const int e = blockIdx.x, l = blockIdx.y, tid = threadIdx.x;
  const int tiles = l == 2 ? o_tiles : hidden / 32, kg = l == 0 ? kg0 : hidden / 8;
  const size_t woff = l == 0 ? off0 : (l == 1 ? off1 : off2), boff = l == 0 ? offb0 : (l == 1 ? offb1 : offb2);
  const float *w = blob + woff + e * pack_floats(tiles, kg);
  const float *b = blob + boff + (size_t)e * tiles * 32;
  float wmax = 0.0f, l1 = 0.0f, bmax = 0.0f;
  if (tid < tiles * 32) {
    const int tile = tid >> 5, r = tid & 31;
    for (int g = 0; g < kg; ++g)
      for (int h = 0; h < 2; ++h) {
        const f32x4 v = *reinterpret_cast<const f32x4 *>(w + pack_index_tile(tile, r, 8 * g + 4 * h, kg));
        for (int s = 0; s < 4; ++s) { const float a = fabsf(v[s]); wmax = fmaxf(wmax, a); l1 += a; }
      }
    bmax = fabsf(b[tid]);
  }
  __shared__ float red[3][kThreadsH];
  red[0][tid] = wmax; red[1][tid] = l1; red[2][tid] = bmax;
  __syncthreads();
  for (int st = kThreadsH / 2; st > 0; st >>= 1) {
    if (tid < st)
      for (int q = 0; q < 3; ++q) red[q][tid] = fmaxf(red[q][tid], red[q][tid + st]);
    __syncthreads();
  }
  if (tid == 0) {
    float *o = stats + (size_t)e * NSTAT + 4 * l;
    o[0] = pow2_lift(red[0][0]); o[1] = red[1][0]; o[2] = red[2][0]; o[3] = red[0][0];
  }
}

// ---- fp32 pack -> two f16 images [n-tile][k-slab][piece 2][lane 64][8 halves] -------------------------------------------
// mode 0 / 1: v_mfma_f32_32x32x16_f16 A fragments, 32-wide n-tiles, 16-deep slabs.  Lane (r, h), element j of slab s holds
// W[n = 32 tile + r][k = 16 s + 8 h + j] * scale.  1 (perm; policy / critic output layers: the B operand is a 32x32
// accumulator tile, whose register i of lane half h is hidden unit (i & 3) + 8 (i >> 2) + 4 h of the tile): slab s covers
// registers 8 (s & 1) .. + 7 of hidden n-tile s >> 1, i.e. k = 32 (s >> 1) + (i & 3) + 8 (i >> 2) + 4 h with i = 8 (s & 1) + j.
// mode 2 / 3: v_mfma_f32_16x16x32_f16 A fragments, 16-wide n-tiles, 32-deep slabs.  Lane (r, g) = (l & 15, l >> 4), element
// j of slab s holds W[n = 16 tile + r][k = 32 s + 8 pi(g) + j], pi = (0, 2, 1, 3) (the B reads of ens_h3's layer 1 take the
// k chunks of an image row in that order: conflict-free ds_read_b128, see read_b there).  3 (ens_h3's output layer: the B
// operand is two 16x16 accumulator tiles of hidden units, register i of lane group g of tile u = unit 16 u + 4 g + i):
// k = 32 s + 16 (j >> 2) + 4 g + (j & 3).
// n beyond the source's tiles and k beyond the pack are zero.
__global__ void h3_pack_kernel(const float *src, size_t src_stride, int kg, int src_tiles, f16x8 *dst, size_t dst_stride,
                               int n_tiles, int slabs, int members, const float *stats, int layer, int mode) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long per = (long)IMAGE_UNITS(n_tiles, slabs, 1);
  if (idx >= per * members) return;
  const int e = (int)(idx / per);
  const int rem = (int)(idx - (long)e * per);
  const int lane = rem & 63, s = (rem >> 6) % slabs, tile = (rem >> 6) / slabs;
  const bool m16 = mode >= 2;
  const int n = m16 ? 16 * tile + (lane & 15) : 32 * tile + (lane & 31);
  const int r = n & 31, g = m16 ? lane >> 4 : lane >> 5;
  const float scale = stats[(size_t)e * NSTAT + 4 * layer];
  const float *sp = src + (size_t)e * src_stride;
  f16x8 p1, p2;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    int k;
    if (mode == 0) k = 16 * s + 8 * g + j;
    else if (mode == 1) {
      const int i = 8 * (s & 1) + j;
      k = 32 * (s >> 1) + (i & 3) + 8 * (i >> 2) + 4 * g;
    } else if (mode == 2) k = 32 * s + 8 * ((g & 1) * 2 + (g >> 1)) + j;
    else k = 32 * s + 16 * (j >> 2) + 4 * g + (j & 3);
    float v = 0.0f;
    if ((n >> 5) < src_tiles && (k >> 3) < kg) v = sp[pack_index_tile(n >> 5, r, k, kg)];
    _Float16 q1, q2;
    split_h(v * scale, q1, q2);
    p1[j] = q1; p2[j] = q2;
  }
  f16x8 *d = dst + (size_t)e * dst_stride + IMAGE_INDEX(tile, slabs, s, 2, 0) + lane;
  d[0] = p1; d[kImageLanes] = p2;
}

// compile-time loop: f(integral_constant<int, I>) for I in [I0, N) -- indices of register arrays must be constants
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F &&f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

// The item loop's barriers order LDS traffic only (images, partial sums, staging tiles; nothing stored to global memory is read
// back inside the kernel), so they are lds_barrier()s: a __syncthreads() would wait for every global access in flight -- the
// output stores of the previous unit (a write acknowledgement from HBM), the next item's input rows and row indices, the
// weight fragments requested a slab ahead.

// The stage of an item in pieces (stage_piece in the kernel); pieces 0 .. kReqEarly - 1 only request (in the old order they
// travel behind the tail).  Where the pieces stand in the last fused step (slot of 24 MFMAs, MFMA i of the slot): slots 0 / 1
// request; slots 2 .. 4 (a memory round trip under load) carry nothing but the rounds of the W0 chunks and the constants
// that wait for the biases alone -- nothing else of the stage is independent of the raw rows; slots 5 .. 7 consume them, a
// piece behind every second MFMA (the row scales' divisions get two gaps each).  Measured: with the rows consumed from
// slot 4 on a 100 k-row forward is 1.2 % slower than with this table (1 084 against 1 071 us), with the rows REQUESTED behind the
// ring's last loads of the step (slot 4) and consumed in slot 7 as slow as the old order -- vmcnt counts in order, so every
// wait for a weight fragment requested after the rows waits for the rows too.
constexpr int kPieces = 24, kReqEarly = 5;
__host__ __device__ constexpr int piece_at(int slot, int i) {
  if (i % 2 != 0) return -1;
  const int k = i / 2;
  if (slot == 0) return k % 3 == 0 ? k / 3 : -1;                                                // raw rows: 0 .. 3
  if (slot == 1) return k == 0 ? 4 : (k == 2 ? 5 : (k == 4 ? 6 : -1));                          // biases, head, W0 round 0
  if (slot == 3) return k == 4 ? 13 : -1;                                                       // W0 round 1
  if (slot == 4) return k == 1 ? 7 : -1;                                                        // biases, head constants -> LDS
  if (slot == 5) return k == 4 ? 20 : (k >= 6 && k < 10 ? 2 + k : -1);                          // W0 round 2; scaler: 8 .. 11
  // row maximum + lift 12, row scales 14 / 15, split 16 .. 19, x image 21
  if (slot == 6) return k == 0 ? 12 : (k == 1 ? 14 : (k == 3 ? 15 : (k == 5 ? 16 : (k >= 7 && k <= 9 ? 10 + k : (k == 10 ? 21 : -1)))));
  if (slot == 7) return k < 2 ? 22 + k : -1;                                                    // the last KB of W0, the next row index
  return -1;
}

// The image instances (IMG): the split x image and the rows' maxima come ready from h3_ximage_kernel, so pieces 0 .. 3,
// 8 .. 12, 16 .. 19 and 21 of the table above do not exist.  What takes their numbers: 0 / 1 request the image (LDS-DMA,
// two 1-KiB pieces per wave each), 2 requests the row's maximum.  They stand behind the ring's last load of the step (slot 3,
// MFMA 23) and behind the MFMA that waits for its last half (slot 4, MFMA 6): no wait for a weight fragment has them in
// front of it.  Piece 22 ends with the wait for the image; only the next row index is requested after it.
__host__ __device__ constexpr int piece_at_img(int slot, int i) {
  if (i % 2 != 0) return -1;
  const int k = i / 2;
  if (slot == 1) return k == 0 ? 4 : (k == 2 ? 5 : (k == 4 ? 6 : -1));                          // biases, head, W0 round 0
  if (slot == 3) return k == 4 ? 13 : -1;                                                       // W0 round 1
  if (slot == 4) return k == 1 ? 7 : (k == 3 ? 2 : (k == 5 ? 0 : (k == 7 ? 1 : -1)));           // constants -> LDS; maximum, image
  if (slot == 5) return k == 4 ? 20 : -1;                                                       // W0 round 2
  if (slot == 6) return k == 1 ? 14 : (k == 3 ? 15 : -1);                                       // row scales
  if (slot == 7) return k < 2 ? 22 + k : -1;                                                    // the last KB of W0 + the image's wait, the next row index
  return -1;
}
__host__ __device__ constexpr int piece_of(bool img, int slot, int i) { return img ? piece_at_img(slot, i) : piece_at(slot, i); }

struct H3Args {
  MlpKernelArgs m;
  const f16x8 *w0, *w1, *w2;
  size_t w0_stride, w1_stride, w2_stride;   // per member, in 16-B units
  const float *stats;                        // [E][NSTAT]
  int item0;                                 // first item of this launch (a launch may carry a suffix of the item list)
  const char *ximg;                          // image instances: the tile blocks h3_ximage_kernel wrote
};

// ---- the x image of a launch's rows, once per row instead of once per (member, row) ----------------------------------
// One block per 128-row tile of the launch's row list, in the layout of the kernel's LDS x image: [piece 2][128][XSTR]
// halves, then the rows' max |x| as 128 floats.  The arithmetic is the stage's (pieces 0 .. 3, 8 .. 12, 16 .. 19, 21 of
// stage_piece, same thread-to-element map): nothing of it depends on the member.  Rows beyond the row count and the 8 pad
// halves of every row are zeros, so every byte of a block is written.  grid = tiles, 512 threads.
__host__ __device__ constexpr int ximg_block_bytes(int S0) { return ximg_bytes(S0, 4) + 128 * 4; }
template <int S0>
__global__ __launch_bounds__(kThreadsH) void h3_ximage_kernel(const MlpKernelArgs p, char *img) {
  static_assert(S0 < 4 && ximg_block_bytes(S0) % 512 == 0, "h3_ximage_kernel: pad halves are written by the thread behind the row's last element");
  constexpr int XSTR = 16 * S0 + 8, TPR = Geo<4>::TPR, KPT = Geo<4>::KPT;
  const int n_rows = p.n_rows_dev ? *p.n_rows_dev : p.n_rows;
  const int tid = threadIdx.x, xb = tid / TPR, xc = tid % TPR;
  __shared__ float mu_l[64], isig_l[64];      // the input scaler as the stage holds it: mu, 1 / sigma
  if (tid < 64) {
    mu_l[tid] = (p.in_mu && tid < p.in_dim) ? p.in_mu[tid] : 0.0f;
    isig_l[tid] = (p.in_mu && tid < p.in_dim) ? 1.0f / p.in_sig[tid] : 1.0f;
  }
  __syncthreads();
  const int rr = blockIdx.x * 128 + xb;
  const bool ok = rr < n_rows;
  int v = ok ? rr : 0;
  if (p.row_idx) v = p.row_idx[v];
  const float *orow = p.obs + (size_t)v * p.obs_dim;
  const float *arow = p.act_dim > 0 ? p.act + (size_t)v * p.act_dim - p.obs_dim : orow;
  float x[KPT];
  float m = 0.0f;
#pragma unroll
  for (int u = 0; u < KPT; ++u) {
    const int k = KPT * xc + u;
    const bool in_obs = k < p.obs_dim, in_act = !in_obs & (k < p.in_dim);
    const float *base = in_act ? arow : orow;
    const float raw = base[(in_obs | in_act) ? k : 0];
    float xv = (raw - mu_l[k]) * isig_l[k];
    xv = ((k < p.in_dim) & ok) ? xv : 0.0f;
    x[u] = xv;
    m = fmaxf(m, fabsf(xv));
  }
#pragma unroll
  for (int o = 1; o < TPR; o <<= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  const float t0 = pow2_lift(m);
  char *blk = img + (size_t)blockIdx.x * ximg_block_bytes(S0);
  _Float16 *d1 = reinterpret_cast<_Float16 *>(blk) + (size_t)xb * XSTR + KPT * xc, *d2 = d1 + (size_t)128 * XSTR;
  if (KPT * xc < 16 * S0) {
#pragma unroll
    for (int w = 0; w < KPT / 8; ++w) {
      f16x8 h1, h2;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        _Float16 a, b;
        split_h(x[8 * w + j] * t0, a, b);
        h1[j] = a; h2[j] = b;
      }
      reinterpret_cast<f16x8 *>(d1)[w] = h1; reinterpret_cast<f16x8 *>(d2)[w] = h2;
    }
  } else if (KPT * xc == 16 * S0) {
    f16x8 z;
#pragma unroll
    for (int j = 0; j < 8; ++j) z[j] = (_Float16)0.0f;
    *reinterpret_cast<f16x8 *>(d1) = z; *reinterpret_cast<f16x8 *>(d2) = z;
  }
  if (xc == 0) reinterpret_cast<float *>(blk + ximg_bytes(S0, 4))[xb] = m;
}

// S0: k-slabs of the input layer (in_pad <= 16 S0); OTP: output n-tiles, 2 or 4 (2 out_dim <= 32 OTP); RT: 32-row tiles per item
// IMG: the x image comes from h3_ximage_kernel's tile blocks by LDS-DMA (stage-ahead instances at RT == 4 only)
template <int S0, int OTP, int RT, bool IMG = false>
__global__ __launch_bounds__(kThreadsH, 2) void ens_h3_kernel(const H3Args a) {
  using G = Geo<RT>;
  constexpr int ROWSH = G::ROWS, NTC = G::NTC, CK = G::CK, NCH = G::NCH, SLC = G::SLC, CSTR = G::CSTR, TPR = G::TPR,
                KPT = G::KPT, DH = G::DH, NPH = G::NPH, CBUF_BYTES = G::CBUF_BYTES;
  constexpr int XSTR = 16 * S0 + 8;
  constexpr int NPASS = OTP / 2;         // output tiles are taken two at a time
  constexpr int NUNIT = RT * NPASS;      // (row tile, pass) units of the tail
  constexpr int O_PAD = 32 * OTP;
  constexpr int W0P = NTC * S0 * 2;      // 1-KB pieces of one W0 chunk
  constexpr bool AHEAD = stage_ahead(S0, RT);
  static_assert(!IMG || (AHEAD && RT == 4), "ens_h3: the image instances are the stage-ahead ones at 128 rows");
  constexpr int NXP = ximg_bytes(S0, RT) / 1024;     // 1-KiB pieces of the x image
  static_assert(!IMG || ximg_bytes(S0, RT) % 1024 == 0, "ens_h3: the x image in whole LDS-DMA pieces");
  const MlpKernelArgs &p = a.m;
  extern __shared__ f32x4 smem4[];
  char *smem = reinterpret_cast<char *>(smem4);
  _Float16 *cbuf = reinterpret_cast<_Float16 *>(smem);                               // [2][2][128][CSTR]
  _Float16 *ximg = reinterpret_cast<_Float16 *>(smem + off_ximg(S0, RT));            // [2][128][XSTR]
  f16x8 *w0buf = reinterpret_cast<f16x8 *>(smem + off_ximg(S0, RT) + ximg_bytes(S0, RT));   // [2][W0P][64] (RT == 4 only)
  constexpr bool PB2 = !AHEAD;           // two buffers of partial outputs (by unit parity)
  f32x4 *pbuf = reinterpret_cast<f32x4 *>(smem);                                     // [PB2 ? 2 : 1][8 waves][2 tiles][4][64] x 16 B
  float *stg = reinterpret_cast<float *>(smem + (PB2 ? 2 : 1) * PBUF_BYTES);         // [2][32][SWS]
  float *cst = reinterpret_cast<float *>(smem + off_const(S0, RT));
  // the per-item constants: copy `par` (item parity within the workgroup's list; one copy where nothing is staged ahead)
  struct Cst { float *bias0, *bias1, *hc_a, *hc_c; int *rowidx; float *r_inv0, *r_t1, *r_inv1, *r_t2, *r_inv2; };
  auto cst_of = [&](int par) {
    Cst c;
    c.bias0 = cst + (AHEAD ? par : 0) * ITEM_FLOATS; c.bias1 = c.bias0 + HIDH; c.hc_a = c.bias0 + 2 * HIDH; c.hc_c = c.hc_a + 128;
    c.rowidx = reinterpret_cast<int *>(c.hc_c + 128);
    c.r_inv0 = c.hc_c + 256; c.r_t1 = c.r_inv0 + 128; c.r_inv1 = c.r_t1 + 128; c.r_t2 = c.r_inv1 + 128; c.r_inv2 = c.r_t2 + 128;
    return c;
  };
  float *in_mu_l = cst + (AHEAD ? 2 : 1) * ITEM_FLOATS, *in_sig_l = in_mu_l + 64;

  const int n_rows = p.n_rows_dev ? *p.n_rows_dev : p.n_rows;
  const int out = p.out_dim;
  if (!IMG && threadIdx.x < 64) {   // input scaler, once per workgroup (TensorStandardScaler.transform, models/pens/utils.py:156)
    const int k = threadIdx.x;
    in_mu_l[k] = (p.in_mu && k < p.in_dim) ? p.in_mu[k] : 0.0f;
    in_sig_l[k] = (p.in_mu && k < p.in_dim) ? 1.0f / p.in_sig[k] : 1.0f;      // 1 / sigma: see the stage
  }
  __syncthreads();

  // The workgroup's items: item0 + blockIdx.x + j gridDim.x, without those whose rows all lie beyond the (device) row count.
  auto next_alive = [&](int it) {     // (uniform)
    while (it < p.n_items) {
      const int e2 = it / p.tiles;
      if ((it - e2 * p.tiles) * ROWSH < n_rows) break;
      it += gridDim.x;
    }
    return it;
  };
  int rr_pre = -1;      // row index of this thread's row of the item that is staged next
  int tile_pre = 0;     // (image instances) its row tile
  auto fetch_row = [&](int it, int tid) {
    const int xb = tid / TPR;
    const int e2 = it / p.tiles;
    if constexpr (IMG) tile_pre = it < p.n_items ? it - e2 * p.tiles : 0;
    const int rr = (it - e2 * p.tiles) * ROWSH + xb;
    const bool ok = it < p.n_items && rr < n_rows;
    int v = ok ? rr : 0;
    if (p.row_idx) v = p.row_idx[v];
    rr_pre = ok ? v : -1;
  };

  // ---- the stage of an item: constants, per-row scales, the split input image, the first two W0 chunks -> LDS, in
  // kPieces pieces of at most ~20 issue cycles (the x loads' address arithmetic and the row scales' divisions somewhat more).
  // The first item of a workgroup runs them in a row in front of its layers; every later item's pieces are dealt out between
  // the layer-1 MFMAs of its predecessor's last fused step (step(), STG), which has no chunk to produce and whose x image,
  // W0 ring and other constants copy nobody reads any more.  Pieces 0 .. 6 only request: raw rows (clamped addresses, the
  // selection happens on the values: a load inside a per-element branch makes hipcc wait for it there), biases | head
  // constants, the member's statistics, the first KB per wave of W0 chunks 0 / 1 (they pass through four registers, W0R
  // rounds).  The others consume, behind the counted vmcnt waits hipcc places (the weight ring's loads stay in flight).
  // An empty volatile asm after a piece keeps it where it stands.
  constexpr int W0R = G::W0_LDS ? (2 * W0P + kWavesH - 1) / kWavesH : 1;
  constexpr int GQ = KPT / 4;        // input elements per piece
  struct StageRegs {
    float x[KPT];
    float b0, b1, b2, hs, hm, hl;    // biases of this thread's hidden unit / output, output scaler
    float st[7];                     // the member's statistics (uniform)
    f16x8 w0r[W0R];
    float m, t0, t1, t2;
    unsigned q1[KPT / 2], q2[KPT / 2];   // the two f16 pieces, packed
  };
  auto stage_piece = [&](auto KC, auto FRONTC, StageRegs &s, const int es, const Cst &c, const int tid, const int it_next) {
    constexpr int K = decltype(KC)::value;
    constexpr bool FRONT = decltype(FRONTC)::value;
    const int xb = tid / TPR, xc = tid % TPR;
    if constexpr (IMG && (K < 4 || (K >= 8 && K <= 12) || (K >= 16 && K <= 19) || K == 21)) {
      // The ready image: LDS-DMA, 16 B per lane, 1-KiB wave pieces dealt over the eight waves (destination = wave-uniform
      // base + 16 lane), and the row's maximum.  The DMA is an asm statement: hipcc puts a wait for a DMA it knows of in
      // front of the wave's next LDS access, which here is the B fragment of the next (slab, row tile) position.  What it
      // does not know of it does not count: its counted waits for later loads only wait for more than they need.
      const char *blk = a.ximg + (size_t)tile_pre * ximg_block_bytes(S0);
      if constexpr (K < 2) {
        const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        const unsigned lds_x = (unsigned)(unsigned long)(__attribute__((address_space(3))) char *)(smem + off_ximg(S0, RT));
#pragma unroll
        for (int u = 2 * K; u < 2 * K + 2; ++u) {
          const int j = wave + kWavesH * u;
          if (kWavesH * u < NXP && j < NXP) {     // (wave-uniform)
            const char *g = blk + (size_t)j * 1024 + lane * 16;
            const unsigned d = __builtin_amdgcn_readfirstlane(lds_x + j * 1024);
            unsigned keep;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(g), "s"(d) : "memory");
          }
        }
        static_assert(NXP <= 4 * kWavesH, "ens_h3: pieces 0 / 1 request the whole x image");
      } else if constexpr (K == 2) {
        s.m = reinterpret_cast<const float *>(blk + ximg_bytes(S0, RT))[xb];
      }
    } else if constexpr (K < 4) {
      const int rr = rr_pre >= 0 ? rr_pre : 0;
      const float *orow = p.obs + (size_t)rr * p.obs_dim;
      const float *arow = p.act_dim > 0 ? p.act + (size_t)rr * p.act_dim - p.obs_dim : orow;
#pragma unroll
      for (int u = GQ * K; u < GQ * K + GQ; ++u) {
        // (selects on values, not on address expressions: the load stays unconditional)
        const int k = KPT * xc + u;
        const bool in_obs = k < p.obs_dim, in_act = !in_obs & (k < p.in_dim);
        const float *base = in_act ? arow : orow;
        const int off = (in_obs | in_act) ? k : 0;
        s.x[u] = base[off];
      }
    } else if constexpr (K == 4) {
      s.b0 = p.b0[(size_t)es * HIDH + tid];
      s.b1 = p.b1[(size_t)es * HIDH + tid];
      const int ob = p.o_tiles * 32;
      s.b2 = p.b2[(size_t)es * ob + (tid < ob ? tid : 0)];
    } else if constexpr (K == 5) {
      s.hs = 1.0f; s.hm = 0.0f; s.hl = 0.0f;
      if (p.out_mu) {     // (uniform)
        const int ia = tid < out ? tid : out - 1, il = tid < out ? 0 : (tid < 2 * out ? tid - out : out - 1);
        s.hs = p.out_sig[ia]; s.hm = p.out_mu[ia]; s.hl = p.out_lsig2[il];
      }
      const float *st = a.stats + (size_t)es * NSTAT;
      s.st[0] = st[0]; s.st[1] = st[1]; s.st[2] = st[2]; s.st[3] = st[4]; s.st[4] = st[5]; s.st[5] = st[6]; s.st[6] = st[8];
    } else if constexpr (K == 6 || K == 13 || K == 20 || K == 22) {
      // The W0 chunks.  In front of an item: every KB of the wave requested at once (piece 6), written at the end (piece 22),
      // as many registers as rounds.  Staged ahead: in rounds through four registers -- round u writes what round u - 1
      // requested and requests the next KB.
      if constexpr (G::W0_LDS) {
        const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        const f16x8 *w0s = a.w0 + (size_t)es * a.w0_stride;
        auto get = [&](f16x8 &x, int u) { const int j = wave + kWavesH * u; x = w0s[(size_t)(j < 2 * W0P ? j : 0) * 64 + lane]; };
        auto put = [&](const f16x8 &x, int u) { const int j = wave + kWavesH * u; if (j < 2 * W0P) w0buf[(size_t)j * 64 + lane] = x; };
        if constexpr (FRONT) {
#pragma unroll
          for (int u = 0; u < W0R; ++u) {
            if constexpr (K == 6) get(s.w0r[u], u);
            if constexpr (K == 22) put(s.w0r[u], u);
          }
        } else {
          constexpr int u = K == 6 ? 0 : (K == 13 ? 1 : (K == 20 ? 2 : 3));
          static_assert(W0R <= 3, "ens_h3: rounds of the W0 chunks");
          if constexpr (u >= 1 && u <= W0R) put(s.w0r[0], u - 1);
          if constexpr (u < W0R) get(s.w0r[0], u);
        }
      }
      // the x image has landed before the barrier that ends the stage (lds_barrier waits for LDS instructions only); every
      // other load requested so far has been consumed, the next row index is requested behind this
      if constexpr (IMG && K == 22) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else if constexpr (K == 7) {
      c.bias0[tid] = s.b0 * kLog2e;      // (the epilogues work on z log2(e): f16_split.h)
      c.bias1[tid] = s.b1 * kLog2e;
      if (tid < O_PAD) {
        // y = A_n z + B_n with z = o + b2_n; n < out: mean = sig z + mu; out <= n < 2 out: var = exp(z + 2 log sig)
        // (models/pens/pe.py:815-835)
        const bool is_mean = tid < out, is_var = !is_mean & (tid < 2 * out);
        float A = is_var ? 1.0f : 0.0f, Bc = is_var ? s.hl : 0.0f;
        A = is_mean ? s.hs : A; Bc = is_mean ? s.hm : Bc;
        c.hc_a[tid] = A;
        c.hc_c[tid] = A * s.b2 + Bc;
      }
    } else if constexpr (K < 12) {
      if constexpr (K == 8) s.m = 0.0f;
#pragma unroll
      for (int u = GQ * (K - 8); u < GQ * (K - 8) + GQ; ++u) {
        const int k = KPT * xc + u;
        // TensorStandardScaler.transform (models/pens/utils.py:156) as (x - mu) (1 / sigma): within an ulp of the division, a
        // tenth of its instructions (sixteen IEEE divisions per thread were a third of the stage)
        float x = (s.x[u] - in_mu_l[k & 63]) * in_sig_l[k & 63];
        const bool keep = (k < p.in_dim) & (rr_pre >= 0);
        x = keep ? x : 0.0f;
        s.x[u] = x;
        s.m = fmaxf(s.m, fabsf(x));
        asm volatile("" : "+v"(s.x[u]));
      }
      asm volatile("" : "+v"(s.m));
    } else if constexpr (K == 12) {
#pragma unroll
      for (int o = 1; o < TPR; o <<= 1) s.m = fmaxf(s.m, __shfl_xor(s.m, o, 64));
      s.t0 = pow2_lift(s.m);
      asm volatile("" : "+v"(s.m), "+v"(s.t0));
    } else if constexpr (K == 14) {
      if (xc == 0) {
        if constexpr (IMG) s.t0 = pow2_lift(s.m);
        const float bound1 = (s.st[1] * s.m + s.st[2]) * 1.001f, t1 = pow2_lift(bound1);
        const float bound2 = (s.st[4] * bound1 + s.st[5]) * 1.001f, t2 = pow2_lift(bound2);
        c.rowidx[xb] = rr_pre;
        c.r_inv0[xb] = 1.0f / (s.st[0] * s.t0);
        c.r_t1[xb] = t1;
        c.r_t2[xb] = t2;
        s.t1 = t1; s.t2 = t2;
      }
    } else if constexpr (K == 15) {
      if (xc == 0) {
        c.r_inv1[xb] = 1.0f / (s.st[3] * s.t1);
        c.r_inv2[xb] = 1.0f / (s.st[6] * s.t2);
      }
    } else if constexpr (K < 20) {
#pragma unroll
      for (int u = GQ * (K - 16); u < GQ * (K - 16) + GQ; ++u) {
        _Float16 h1, h2;
        split_h(s.x[u] * s.t0, h1, h2);
        // (the halves of a dword one after the other: u even first)
        if (u % 2 == 0) { s.q1[u / 2] = __builtin_bit_cast(unsigned short, h1); s.q2[u / 2] = __builtin_bit_cast(unsigned short, h2); }
        else {
          s.q1[u / 2] |= (unsigned)__builtin_bit_cast(unsigned short, h1) << 16;
          s.q2[u / 2] |= (unsigned)__builtin_bit_cast(unsigned short, h2) << 16;
          asm volatile("" : "+v"(s.q1[u / 2]), "+v"(s.q2[u / 2]));
        }
      }
    } else if constexpr (K == 21) {
      if (KPT * xc < 16 * S0) {
        _Float16 *d1 = ximg + (size_t)xb * XSTR + KPT * xc, *d2 = d1 + (size_t)ROWSH * XSTR;
        if constexpr (KPT >= 8) {
#pragma unroll
          for (int v = 0; v < KPT / 8; ++v) {
            u32x4 w1, w2;
#pragma unroll
            for (int u = 0; u < 4; ++u) { w1[u] = s.q1[4 * v + u]; w2[u] = s.q2[4 * v + u]; }
            reinterpret_cast<u32x4 *>(d1)[v] = w1; reinterpret_cast<u32x4 *>(d2)[v] = w2;
          }
        } else {
          *reinterpret_cast<uint2 *>(d1) = make_uint2(s.q1[0], s.q1[1]);
          *reinterpret_cast<uint2 *>(d2) = make_uint2(s.q2[0], s.q2[1]);
        }
      }
    } else {
      fetch_row(it_next, tid);     // the row index of the item after: lands during the layers
    }
  };
#ifdef CMBPO_STAMPS
  unsigned long long t_acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long t_last = __builtin_amdgcn_s_memtime();
  const unsigned long long t_rt0 = __builtin_amdgcn_s_memrealtime();
#endif

  StageRegs sr;       // requests in flight: the first item's, and (old order only) the next item's behind the tail
  // the stage in a row in front of an item's layers: the first item of a workgroup -- every item in the old order
  auto stage_front = [&](int es, const Cst &c, int tid, int it_next) {
    static_for<kReqEarly, kPieces>([&](auto P) { stage_piece(P, std::true_type{}, sr, es, c, tid, it_next); });
    H3_STAMP(0);
    lds_barrier();
    H3_STAMP(1);
  };
  int item = next_alive(a.item0 + blockIdx.x);
  int nxt = next_alive(item + gridDim.x);
  int par = 0;
  if (item < p.n_items) {
    fetch_row(item, threadIdx.x);
    const int e0 = item / p.tiles;
    static_for<0, kReqEarly>([&](auto P) { stage_piece(P, std::true_type{}, sr, e0, cst_of(0), threadIdx.x, 0); });
    if constexpr (AHEAD) stage_front(e0, cst_of(0), threadIdx.x, nxt);
  }

  while (item < p.n_items) {
    // the thread index, re-read inside the loop through an opaque move: everything derived from it is recomputed per
    // item instead of being hoisted out of the loop and parked in scratch (the loop body needs every register)
    int tid = threadIdx.x;
    asm volatile("v_mov_b32 %0, %0" : "+v"(tid));
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hh = lane >> 5;
    const int e = item / p.tiles;
    const int e_nxt = (nxt < p.n_items ? nxt : item) / p.tiles;
    const int nxt2 = next_alive(nxt + gridDim.x);
    const Cst cc = cst_of(par);
    float *const bias0 = cc.bias0, *const bias1 = cc.bias1, *const hc_a = cc.hc_a, *const hc_c = cc.hc_c;
    int *const rowidx = cc.rowidx;
    float *const r_inv0 = cc.r_inv0, *const r_t1 = cc.r_t1, *const r_inv1 = cc.r_inv1, *const r_t2 = cc.r_t2, *const r_inv2 = cc.r_inv2;
    const f16x8 *w0e = a.w0 + (size_t)e * a.w0_stride;
    if constexpr (!AHEAD) stage_front(e, cc, tid, nxt);

    // ---- layers 0 + 1, fused over the 8 chunks of h1 -------------------------------------------------------------------
    const int l0_tn = wave & (NTC - 1), l0_bt = wave / NTC;     // this wave's (n-tile, row-tile) pair of every chunk
    const float inv0_l = r_inv0[32 * l0_bt + r] * kLog2e;
    const float t1_l = pow2_rcp(r_t1[32 * l0_bt + r]) * kLog2e;     // (the epilogue takes 1 / lift)
    const _Float16 *xb0 = ximg + (size_t)(32 * l0_bt + r) * XSTR + 8 * hh;
    // layer-0 operands of one 16-deep slab: W0 fragments of the chunk (LDS copy) and this wave's rows of the x image
    struct L0Ops { f16x8 a1, a2, b1, b2; };
    auto l0_read = [&](L0Ops &o, int cc, int s) {
      // W0 fragments: the chunk's LDS copy when several waves share an n-tile (RT == 4), straight from L2 otherwise (the
      // step after the last chunk computes a chunk nobody reads: any valid address will do)
      const f16x8 *wa = G::W0_LDS ? w0buf + ((size_t)(cc & 1) * W0P + (size_t)l0_tn * S0 * 2 + 2 * s) * 64 + lane
                                  : w0e + (((size_t)(cc < NCH ? cc : NCH - 1) * NTC + l0_tn) * S0 * 2 + 2 * s) * 64 + lane;
      o.a1 = wa[0]; o.a2 = wa[64];
      o.b1 = *reinterpret_cast<const f16x8 *>(xb0 + 16 * s);
      o.b2 = *reinterpret_cast<const f16x8 *>(xb0 + (size_t)ROWSH * XSTR + 16 * s);
    };
    auto l0_store = [&](const Epi4 &s, int cc, int q) {
      _Float16 *c1 = cbuf + (size_t)(cc & 1) * (CBUF_BYTES / 2) + (size_t)(32 * l0_bt + r) * CSTR + 32 * l0_tn + 4 * hh + 8 * q;
      *reinterpret_cast<uint2 *>(c1) = make_uint2(s.q1[0], s.q1[1]);
      *reinterpret_cast<uint2 *>(c1 + (size_t)ROWSH * CSTR) = make_uint2(s.q2[0], s.q2[1]);
    };
    auto l0_bias = [&](int cc, int q) {
      return *reinterpret_cast<const f32x4 *>(bias0 + cc * CK + 32 * l0_tn + 8 * q + 4 * hh);
    };

    // Layer 1 on v_mfma_f32_16x16x32_f16 (the same work as 32x32x16 at less power per FLOP; the chip holds its clock by
    // power): wave w owns hidden units 64 w .. 64 w + 63 as four 16-tiles u x the item's 2 RT 16-row tiles v (128
    // accumulator registers at RT == 4).  Column c of row tile v is item row 16 v + sig(c): sig even for c in {0..3, 12..15},
    // odd for c in {4..11}.  With that and the image row's k chunks taken in the order pi = (0, 2, 1, 3) (h3_pack_kernel, mode
    // 2), the ds_read_b128 of a B fragment is conflict-free: its 16-lane groups are {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}
    // (+32), the row stride is odd in 16-B slots, so a group reads rows of one parity from one chunk and rows of the other
    // from a chunk two slots away (the plain order is 2-way).
    constexpr int VT = 2 * RT;
    const int c16 = lane & 15, g4 = lane >> 4;
    const int sig = c16 < 4 ? 2 * c16 : (c16 < 12 ? 2 * c16 - 7 : 2 * c16 - 16);
    const int pik = 8 * (2 * (g4 & 1) + (g4 >> 1));
    f32x4 acc[4][VT];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int v = 0; v < VT; ++v)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[u][v][i] = 0.0f;
    const f16x8 *w1a = a.w1 + (size_t)e * a.w1_stride + (size_t)(4 * wave) * 16 * 128 + lane;   // [16-tile][slab 16][piece][lane]
    f16x8 A[DH][2][2];     // ring over half slabs: [half % DH][16-tile of the pair][piece]; half h = 2 slab + (tiles 2, 3)
    f16x8 Bt[2][2];        // [position & 1][piece]: the next position's fragments are read during the current one
    auto load_h = [&](f16x8 (&x)[2][2], int h) {
      h = h < 31 ? h : 31;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const f16x8 *q = w1a + ((size_t)(2 * (h & 1) + t) * 16 + (h >> 1)) * 128;
        x[t][0] = q[0]; x[t][1] = q[64];
      }
    };
    auto read_b = [&](f16x8 (&x)[2], const _Float16 *img, int v, int sl) {
      const _Float16 *q = img + (size_t)(16 * v + sig) * CSTR + 32 * sl + pik;
      x[0] = *reinterpret_cast<const f16x8 *>(q);
      x[1] = *reinterpret_cast<const f16x8 *>(q + (size_t)ROWSH * CSTR);
    };
#pragma unroll
    for (int h = 0; h < DH; ++h) load_h(A[h], h);
    {   // chunk 0 of h1: nothing to overlap it with yet
      f32x16 d;
#pragma unroll
      for (int i = 0; i < 16; ++i) d[i] = 0.0f;
#pragma unroll
      for (int s = 0; s < S0; ++s) {
        L0Ops o;
        l0_read(o, 0, s);
        mm3(d, o.a1, o.a2, o.b1, o.b2);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        Epi4 es;
        const f32x4 bv = l0_bias(0, q);
        epi_all<false>(es, d, q, inv0_l, bv, t1_l);
        l0_store(es, 0, q);
      }
    }
    lds_barrier();
    H3_STAMP(2);

    // One step = the 192 layer-1 MFMAs of chunk c -- 16 (slab, row tile) positions of 12, in 8 slots of 24 -- with the
    // production of chunk c + 1 dealt out between them: a wave issues in order, so what stands between two MFMAs runs in the
    // shadow of the first.  Slots 0 .. S0-1 carry the layer-0 MFMAs (32x32x16) of one input slab each (operands read one
    // slot ahead), slots 4 .. 7 one quarter of the swish / lift / split epilogue each, a piece behind every second MFMA.
    // Within a position the MFMAs of tiles 0, 1 come first: the last position of a slab frees that half of the ring 6 MFMAs
    // before the other.  PH = c % NPH: where the ring stands (compile-time register indices).  The last step has no chunk to
    // produce: an instance of its own, which carries the next item's stage in the empty gaps (STG), every piece behind a
    // uniform branch on "there is a next item" (two instances of the step, with and without the stage, cost two hundred
    // spilled registers where they meet again).
    auto step = [&](auto LASTC, const int c, auto PHC) {
      constexpr bool LAST = decltype(LASTC)::value;
      constexpr int PH = decltype(PHC)::value;
      constexpr bool STG = LAST && AHEAD;
      const bool have_next = nxt < p.n_items;
      // the stage's own registers, thread index (an opaque move again: nothing of the stage is computed at the top of the
      // item and carried through the loop) and constants copy
      StageRegs sa;
      int tid_s = 0;
      if constexpr (STG) {
        tid_s = threadIdx.x;
        asm volatile("v_mov_b32 %0, %0" : "+v"(tid_s));
      }
      const Cst cn = cst_of(par ^ 1);
      f16x8 wst;
      const bool stage_w0 = c + 2 < NCH;
      const int cw = stage_w0 ? c + 2 : NCH - 1;
      const _Float16 *img = cbuf + (size_t)(c & 1) * (CBUF_BYTES / 2);
      f32x16 d;
#pragma unroll
      for (int i = 0; i < 16; ++i) d[i] = 0.0f;
      L0Ops l0;
      Epi4 es;
      f32x4 bv = {0.0f, 0.0f, 0.0f, 0.0f};
      read_b(Bt[0], img, 0, 0);
      if constexpr (!LAST) l0_read(l0, c + 1, 0);
      static_for<0, 8>([&](auto SLOTC) {       // (compile-time slot and MFMA index: the stage's pieces are chosen by them)
        constexpr int slot = decltype(SLOTC)::value;
        if (!LAST && slot >= 4) bv = l0_bias(c + 1, slot - 4);
        if constexpr (G::W0_LDS && !LAST) {
          // W0 fragments of chunk c + 2 pass through four registers, one 1-KB piece at a time
          if (slot == 4) wst = w0e[((size_t)cw * W0P + wave) * 64 + lane];
          if (slot == 5 && W0P > kWavesH) {
            if (stage_w0) w0buf[((size_t)(c & 1) * W0P + wave) * 64 + lane] = wst;
            wst = w0e[((size_t)cw * W0P + (wave + kWavesH < W0P ? wave + kWavesH : wave)) * 64 + lane];
          }
        }
        static_for<0, 24>([&](auto IC) {
          constexpr int i = decltype(IC)::value;
          const int pos = 2 * slot + i / 12;                      // position in the (slab, row tile) sequence
          const int sl = pos / VT, v = pos % VT;
          const int u = (i % 12) / 3, term = i % 3;
          const int hl = 2 * sl + (u >> 1);                       // half of this step
          f16x8(&Ah)[2][2] = A[(PH * 2 * SLC + hl) % DH];
          if (i % 12 == 0) {
            if (pos + 1 < 16) read_b(Bt[(pos + 1) & 1], img, (pos + 1) % VT, (pos + 1) / VT);
            if (i == 0) __builtin_amdgcn_sched_barrier(0);
          }
          f32x4 &ac = acc[u][v];
          const f16x8 &b1 = Bt[pos & 1][0], &b2 = Bt[pos & 1][1];
          if (term == 0) ac = __builtin_amdgcn_mfma_f32_16x16x32_f16(Ah[u & 1][1], b1, ac, 0, 0, 0);
          else if (term == 1) ac = __builtin_amdgcn_mfma_f32_16x16x32_f16(Ah[u & 1][0], b2, ac, 0, 0, 0);
          else ac = __builtin_amdgcn_mfma_f32_16x16x32_f16(Ah[u & 1][0], b1, ac, 0, 0, 0);
          if (v == VT - 1 && (i % 12 == 5 || i % 12 == 11) && !(LAST && hl + DH >= 2 * SLC))
            load_h(Ah, c * 2 * SLC + hl + DH);                    // the half's last MFMA: its successor DH halves on
          if (!LAST && slot < S0 && i == 11) {                    // layer-0 MFMAs of input slab `slot`, then the next slab's operands
            mm3(d, l0.a1, l0.a2, l0.b1, l0.b2);
            if (slot + 1 < S0) l0_read(l0, c + 1, slot + 1);
          }
          if (!LAST && slot >= 4 && i % 2 == 0) {
            const int q = slot - 4, k = i / 2;
            if (k == 0) epi_stage<0, true>(es, d, q, inv0_l, bv, t1_l);
            if (k == 2) epi_stage<2, true>(es, d, q, inv0_l, bv, t1_l);
            if (k == 3) epi_stage<3, true>(es, d, q, inv0_l, bv, t1_l);
            if (k == 4) epi_stage<4, true>(es, d, q, inv0_l, bv, t1_l);
            if (k == 5) epi_stage<5, true>(es, d, q, inv0_l, bv, t1_l);
            if (k == 6) epi_stage<6, true>(es, d, q, inv0_l, bv, t1_l);
            if (k == 8) epi_stage<8, true>(es, d, q, inv0_l, bv, t1_l);
            if (k == 9) epi_stage<9, true>(es, d, q, inv0_l, bv, t1_l);
            if (k == 10) l0_store(es, c + 1, q);
          }
          if constexpr (STG && piece_of(IMG, slot, i) >= 0)
            if (have_next) stage_piece(std::integral_constant<int, (piece_of(IMG, slot, i) >= 0 ? piece_of(IMG, slot, i) : 0)>{}, std::false_type{}, sa, e_nxt, cn, tid_s, nxt2);
          __builtin_amdgcn_sched_barrier(0);
        });
      });
      if constexpr (STG) {     // ("slot 8": behind the last MFMA)
        static_for<0, 24>([&](auto IC) {
          constexpr int pc = piece_of(IMG, 8, decltype(IC)::value);
          if constexpr (pc >= 0)
            if (have_next) stage_piece(std::integral_constant<int, (pc >= 0 ? pc : 0)>{}, std::false_type{}, sa, e_nxt, cn, tid_s, nxt2);
        });
      }
      H3_STAMP(4);
      if constexpr (G::W0_LDS && !LAST) {
        if (stage_w0) {
          const int j = W0P > kWavesH ? wave + kWavesH : wave;
          if (j < W0P) w0buf[((size_t)(c & 1) * W0P + j) * 64 + lane] = wst;
        }
      }
      lds_barrier();
      H3_STAMP(5);
    };
    {
      constexpr int NREG = NCH - 1, NFULL = NREG / NPH * NPH;
#pragma unroll 1
      for (int c0 = 0; c0 < NFULL; c0 += NPH)
        static_for<0, NPH>([&](auto P) { step(std::false_type{}, c0 + decltype(P)::value, P); });
      static_for<0, NREG - NFULL>([&](auto P) { step(std::false_type{}, NFULL + decltype(P)::value, P); });
      step(std::true_type{}, NREG, std::integral_constant<int, NREG % NPH>{});
    }
    if constexpr (!AHEAD) {
      // old order: the next item's requests travel behind the tail
      if (nxt < p.n_items) static_for<0, kReqEarly>([&](auto P) { stage_piece(P, std::true_type{}, sr, e_nxt, cc, tid, 0); });
    }
    H3_STAMP(6);

    // ---- tail: h2 -> output layer -> head -> stores, one (32-row tile, pair of output tiles) unit at a time.
    // h2 never leaves the registers: an accumulator tile's hidden units are the next product's k index, so the wave's own 64
    // hidden units (2 32-deep k steps: 16-tiles 2 ks, 2 ks + 1 as one B fragment, W2 packed in that k order, h3_pack_kernel
    // mode 3) are its slice of the output layer's K, and the eight waves' partial outputs are added up through LDS in a fixed
    // order.  The output layer runs on 16x16x32 too: output 16-tile ot = 2 tt + a of the pair tt, 16-row tile vv of the unit.
    const f16x8 *w2w = a.w2 + (size_t)e * a.w2_stride + lane;   // + (16-tile * 16 + slab) * 128 + piece * 64
    auto reduce_unit = [&](int u) {
      // wave w adds up registers 4q .. 4q+3 (q = w & 3) of output tile tt = w >> 2 of this unit over the eight waves,
      // applies the head (models/pens/pe.py:815-835) and leaves the values in the staging tile [row][column of the pair]
      const int rt = u / NPASS, pass = u % NPASS;
      const int tt = wave >> 2, q = wave & 3;
      const f32x4 *pp = pbuf + ((size_t)(PB2 ? u & 1 : 0) * 64 + (size_t)tt * 4 + q) * 64 + lane;
      f32x4 v = pp[0];
#pragma unroll
      for (int wv = 1; wv < kWavesH; ++wv) v += pp[(size_t)wv * 8 * 64];
      const int nl = 32 * tt + 8 * q + 4 * hh, n = 64 * pass + nl;
      const f32x4 ha = *reinterpret_cast<const f32x4 *>(hc_a + n), hc = *reinterpret_cast<const f32x4 *>(hc_c + n);
      const float inv2_l = r_inv2[32 * rt + r];
      float *sg = stg + (size_t)(u & 1) * 32 * SWS + r * SWS + nl;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        float y = ha[s] * (v[s] * inv2_l) + hc[s];
        if (n + s >= out) y = __expf(y);
        sg[s] = y;
      }
    };
    auto store_unit = [&](int u) {
      // a row's means / variances are contiguous runs of `out` floats; lane = column of the pair
      const int rt = u / NPASS, pass = u % NPASS;
      if (NPASS == 1 && (out & 1) == 0) {
        // even widths (every shipped task): 8-byte stores, two rows per instruction -- lanes 0 .. out - 1 carry row A's
        // (mean | var) as `out` float pairs, lanes out .. 2 out - 1 row B's (rows are 8-byte aligned: out 4 bytes a row)
        const int half = lane >= out ? 1 : 0, c = 2 * (lane - half * out);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int rl = wave + kWavesH * (2 * j + half);
          const int rr = rowidx[32 * rt + rl];
          const float *sp = stg + (size_t)(u & 1) * 32 * SWS + rl * SWS + c;
          const float2 y = make_float2(sp[0], sp[1]);
          if (rr >= 0 && lane < 2 * out) {
            const size_t obase = ((size_t)e * p.ld_rows + rr) * out;
            float *dst = c < out ? p.out0 + obase + c : p.out1 + obase + (c - out);
            *reinterpret_cast<float2 *>(dst) = y;
          }
        }
        return;
      }
      // two passes over the output layer, or an odd width: 4-byte lane stores
      const int n = 64 * pass + lane;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int rl = wave + kWavesH * j;
        const int rr = rowidx[32 * rt + rl];
        const float y = stg[(size_t)(u & 1) * 32 * SWS + rl * SWS + lane];
        if (rr >= 0 && n < 2 * out) {
          const size_t obase = ((size_t)e * p.ld_rows + rr) * out;
          if (n < out) p.out0[obase + n] = y;
          else p.out1[obase + (n - out)] = y;
        }
      }
    };
    // h2 of 32-row tile rt: swish, lift, split -- straight into B fragments [16-row tile vv][k step ks][piece]
    auto h2_frag = [&](u32x4 (&bfu)[2][2][2], auto RTI) {
      constexpr int rt = decltype(RTI)::value;
#pragma unroll
      for (int vv = 0; vv < 2; ++vv) {
        const int row = 32 * rt + 16 * vv + sig;
        const float inv1_l = r_inv1[row] * kLog2e;
        const float t2_l = pow2_rcp(r_t2[row]) * kLog2e;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const f32x4 bv = *reinterpret_cast<const f32x4 *>(bias1 + 64 * wave + 16 * u + 4 * g4);
          Epi4 es;
          epi_all<false>(es, acc[u][2 * rt + vv], 0, inv1_l, bv, t2_l);
          bfu[vv][u >> 1][0][2 * (u & 1)] = es.q1[0]; bfu[vv][u >> 1][0][2 * (u & 1) + 1] = es.q1[1];
          bfu[vv][u >> 1][1][2 * (u & 1)] = es.q2[0]; bfu[vv][u >> 1][1][2 * (u & 1) + 1] = es.q2[1];
        }
      }
    };
    // the output layer's MFMAs of k step ks for output tile pair tt: o[a][vv] += W2 fragments w[a][piece] x h2 fragments
    auto out_mm = [&](f32x4 (&o)[2][2], const f16x8 (&w)[2][2], const u32x4 (&bfu)[2][2][2], int ks) {
#pragma unroll
      for (int vv = 0; vv < 2; ++vv) {
        const f16x8 b1 = __builtin_bit_cast(f16x8, bfu[vv][ks][0]), b2 = __builtin_bit_cast(f16x8, bfu[vv][ks][1]);
#pragma unroll
        for (int aa = 0; aa < 2; ++aa) mm3(o[aa][vv], w[aa][0], w[aa][1], b1, b2);
      }
    };
    // partial outputs of unit u to LDS in the layout of a 32x32 tile pair (what reduce_unit reads): lane (r, h), register
    // group q of tile tt = outputs 32 tt + 8 q + 4 h .. + 3 of row r; a 16x16 lane (c, g) of o[tt][a][vv] holds outputs
    // 32 tt + 16 a + 4 g .. + 3 of row 16 vv + sig(c)
    auto put_partials = [&](const f32x4 (&o)[2][2][2], int u) {
      f32x4 *pw = pbuf + ((size_t)(PB2 ? u & 1 : 0) * 64 + (size_t)wave * 8) * 64;
#pragma unroll
      for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int aa = 0; aa < 2; ++aa)
#pragma unroll
          for (int vv = 0; vv < 2; ++vv)
            pw[(size_t)(tt * 4 + 2 * aa + (g4 >> 1)) * 64 + 16 * vv + sig + 32 * (g4 & 1)] = o[tt][aa][vv];
    };
    auto zero_o = [&](f32x4 (&o)[2][2][2]) {
#pragma unroll
      for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int aa = 0; aa < 2; ++aa)
#pragma unroll
          for (int vv = 0; vv < 2; ++vv)
#pragma unroll
            for (int i = 0; i < 4; ++i) o[tt][aa][vv][i] = 0.0f;
    };
    if constexpr (NPASS == 1) {
      // Two output tiles (every shipped task but Humanoid): the wave's 16 W2 fragments (its 2 k steps x 4 output 16-tiles x 2
      // pieces) stay in 64 registers for the four row tiles of the item -- requested once, behind the first row tile's
      // epilogue, instead of once per row tile (a third of the item's L2 -> CU traffic, and an L2 round trip in front of every
      // k step's MFMAs: the chip holds its clock by power, and weight fragments from L2 are what costs most of it beside the MFMAs).
      f16x8 w2r[2][2][2][2];      // [k step][output tile pair][a][piece]
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int ot = 0; ot < 4; ++ot) {
          const f16x8 *q = w2w + ((size_t)ot * 16 + 2 * wave + ks) * 128;
          w2r[ks][ot >> 1][ot & 1][0] = q[0]; w2r[ks][ot >> 1][ot & 1][1] = q[64];
        }
      // The tail as four stages per row tile, A: swish / lift / split of h2 (VALU) -> B: output-layer MFMAs + partial sums to
      // LDS -> [barrier] -> C: sum of the eight waves' partials + head -> D: stores.  Between two barriers a wave runs
      // D(k-2), C(k-1), B(k), A(k+1); with one buffer of partial outputs a barrier of its own stands between B(k)'s MFMAs
      // and its partial sums' writes (every wave has read unit k-1's by then).  Measured (profiles/r03/h3_variants_5.log, _6.log): each stage costs about what its
      // instructions cost alone (A 5.7 %, B 5.1 %, C + D 4.5 % of a forward); giving the two waves of a SIMD opposite orders
      // inside an interval or dealing A(k+1) out between B(k)'s MFMAs changed nothing (1.264 -> 1.269 ms), so the plain
      // order stands.
      u32x4 bfu[2][2][2][2];     // [row tile & 1][16-row tile][k step][piece]
      auto stA = [&](auto RTI) { h2_frag(bfu[decltype(RTI)::value & 1], RTI); };
      auto stB = [&](auto RTI) {
        constexpr int rt = decltype(RTI)::value;
        f32x4 o[2][2][2];
        zero_o(o);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
          for (int tt = 0; tt < 2; ++tt) out_mm(o[tt], w2r[ks][tt], bfu[rt & 1], ks);
        if (!PB2 && rt > 0) lds_barrier();
        put_partials(o, rt);
      };
      stA(std::integral_constant<int, 0>{});
      static_for<0, RT + 2>([&](auto KI) {
        constexpr int k = decltype(KI)::value;      // interval k: D(k - 2), C(k - 1), B(k), A(k + 1)
        if constexpr (k >= 2 && k - 2 < RT) store_unit(k - 2);
        if constexpr (k >= 1 && k - 1 < RT) reduce_unit(k - 1);
        if constexpr (k < RT) stB(std::integral_constant<int, (k < RT ? k : 0)>{});
        if constexpr (k + 1 < RT) stA(std::integral_constant<int, (k + 1 < RT ? k + 1 : 0)>{});
        H3_STAMP(7);
        if constexpr (k + 1 < RT + 2) lds_barrier();
        H3_STAMP(8);
      });
    } else {
      // four output tiles (Humanoid): per row tile two passes over the output layer, the W2 fragments of one (k step, tile
      // pair) stage in flight behind the MFMAs of the previous
      static_for<0, RT>([&](auto RTI) {
        constexpr int rt = decltype(RTI)::value;
        f16x8 wf[2][2][2];       // [ping-pong][a][piece]
        auto load_w2 = [&](f16x8 (&x)[2][2], int pass, int st) {   // stage st = 2 ks + tt
#pragma unroll
          for (int aa = 0; aa < 2; ++aa) {
            const f16x8 *q = w2w + ((size_t)(4 * pass + 2 * (st & 1) + aa) * 16 + 2 * wave + (st >> 1)) * 128;
            x[aa][0] = q[0]; x[aa][1] = q[64];
          }
        };
        load_w2(wf[0], 0, 0);
        u32x4 bfu[2][2][2];
        h2_frag(bfu, RTI);
#pragma unroll
        for (int pass = 0; pass < NPASS; ++pass) {
          const int u = rt * NPASS + pass;
          f32x4 o[2][2][2];
          zero_o(o);
#pragma unroll
          for (int st = 0; st < 4; ++st) {
            if (st < 3 || pass + 1 < NPASS) load_w2(wf[(st & 1) ^ 1], st == 3 ? pass + 1 : pass, (st + 1) & 3);
            out_mm(o[st & 1], wf[st & 1], bfu, st >> 1);
          }
          if (!PB2 && u > 0) lds_barrier();     // one buffer of partial outputs: every wave has summed unit u - 1's
          put_partials(o, u);
          H3_STAMP(7);
          lds_barrier();       // unit u's partials are complete; unit u - 1's staging tile too
          H3_STAMP(8);
          if (u > 0) store_unit(u - 1);
          reduce_unit(u);
          H3_STAMP(9);
        }
      });
      lds_barrier();
      store_unit(NUNIT - 1);
    }
    H3_STAMP(10);
    lds_barrier();     // the tail's buffers are the next item's chunk images (old order: and its stage's x image)
    H3_STAMP(11);
    item = nxt; nxt = nxt2; par ^= 1;
  }  // persistent item loop
#ifdef CMBPO_STAMPS
  if (p.stamps && threadIdx.x == 0) {
    for (int k = 0; k < 12; ++k) p.stamps[(size_t)blockIdx.x * 16 + k] = t_acc[k];
    p.stamps[(size_t)blockIdx.x * 16 + 12] = __builtin_amdgcn_s_memrealtime() - t_rt0;
  }
#endif
}

}  // namespace

// ---- host side -------------------------------------------------------------------------------------------------------
// (re)builds the statistics and the two f16 images from the handle's fp32 packs when they changed since the last build
static int ensure_h3(cmbpo_mlp *m, hipStream_t s) {
  const int H = m->hidden, E = m->ensemble;
  const int S0 = m->h3_s0, OTP = m->h3_otp;
  const int slabs[3] = {S0, H / 32, H / 32};        // layer 0: 32x32x16 fragments; layers 1, 2: 16x16x32 (pack modes 2, 3)
  const int tiles[3] = {H / 32, H / 16, 2 * OTP};
  if (m->d_h3 == nullptr) {
    size_t off = 0;
    for (int l = 0; l < 3; ++l) {
      m->h3_stride[l] = IMAGE_UNITS(tiles[l], slabs[l], 2);
      m->h3_off[l] = off;
      off += m->h3_stride[l] * E;
    }
    m->h3_stats_off = off;    // in 16-B units
    const size_t bytes = off * 16 + (size_t)E * NSTAT * sizeof(float);
    if (hipMalloc(&m->d_h3, bytes) != hipSuccess) {
      (void)hipGetLastError();
      m->d_h3 = nullptr;
      cmbpo_set_error("ens_h3: hipMalloc of the f16 weight images failed");
      return CMBPO_ENOMEM;
    }
    m->h3_version = ~0ul;
  }
  if (m->h3_version == m->pack_version) return CMBPO_OK;
  float *stats = reinterpret_cast<float *>(reinterpret_cast<char *>(m->d_h3) + m->h3_stats_off * 16);
  cmbpo_internal_f16_stats(m, stats, s);
  for (int l = 0; l < 3; ++l)
    cmbpo_internal_f16_pack(m, l, reinterpret_cast<f16x8 *>(m->d_h3) + m->h3_off[l], m->h3_stride[l], tiles[l], slabs[l],
                            l == 0 ? 0 : l + 1, stats, s);
  CMBPO_HIP_CHECK(hipGetLastError());
  m->h3_version = m->pack_version;
  return CMBPO_OK;
}

// shared with critic_f16.hip
void cmbpo_internal_f16_stats(const cmbpo_mlp *m, float *stats, hipStream_t s) {
  hipLaunchKernelGGL(h3_stats_kernel, dim3(m->ensemble, 3), dim3(kThreadsH), 0, s, m->d_blob, m->off_wp0, m->off_wp1, m->off_wp2,
                     m->off_b0, m->off_b1, m->off_b2, m->in_pad / 8, m->o_tiles, m->hidden, stats);
}
void cmbpo_internal_f16_pack(const cmbpo_mlp *m, int layer, void *dst, size_t dst_stride, int n_tiles, int slabs, int perm,
                             const float *stats, hipStream_t s) {
  const long total = (long)(IMAGE_UNITS(n_tiles, slabs, 1) * m->ensemble);
  hipLaunchKernelGGL(h3_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, m->pack(layer), m->pack_floats(layer),
                     m->pack_kg(layer), m->pack_tiles(layer), reinterpret_cast<f16x8 *>(dst), dst_stride, n_tiles, slabs, m->ensemble,
                     stats, layer, perm);
}

static int g_h3_rt = 0;   // 0: by row count; 1 / 2 / 4 forces it
extern "C" int cmbpo_set_ens_f16_row_tiles(int rt) {
  CMBPO_REQUIRE(rt == 0 || rt == 1 || rt == 2 || rt == 4, "cmbpo_set_ens_f16_row_tiles: 0 (by row count), 1, 2 or 4");
  g_h3_rt = rt;
  return CMBPO_OK;
}

// rows from which the main launch at 128-row items takes the x image of h3_ximage_kernel: 0 = from the row count at which
// every workgroup of that launch has at least two items (the first item of a workgroup is staged in front of its layers
// either way, and the image costs a launch); < 0 never; 1 whenever the main launch has 128-row items
static int g_h3_img_min_rows = 0;
extern "C" int cmbpo_set_ens_f16_image_min_rows(int rows) {
  g_h3_img_min_rows = rows;
  return CMBPO_OK;
}

// room for the x image of n_rows rows in the handle: at least the caller's branch slots, so that it is allocated once
static int ensure_ximg(cmbpo_mlp *m, int n_rows, int ld_rows, size_t block_bytes) {
  const size_t need = (size_t)cmbpo_ceil_div(n_rows, 128);
  if (m->d_ximg != nullptr && m->ximg_tiles >= need && m->ximg_block == block_bytes) return CMBPO_OK;
  if (m->d_ximg) (void)hipFree(m->d_ximg);      // synchronises: nothing in flight still reads the old block
  m->d_ximg = nullptr; m->ximg_tiles = 0;
  const size_t slots = ld_rows > 0 ? (size_t)cmbpo_ceil_div(ld_rows, 128) : 0;
  const size_t tiles = need > slots ? need : slots;
  if (hipMalloc(&m->d_ximg, tiles * block_bytes) != hipSuccess) {
    (void)hipGetLastError();
    m->d_ximg = nullptr;
    cmbpo_set_error("ens_h3: hipMalloc of the input image (%zu B) failed", tiles * block_bytes);
    return CMBPO_ENOMEM;
  }
  m->ximg_tiles = tiles; m->ximg_block = block_bytes;
  return CMBPO_OK;
}

bool cmbpo_internal_h3_eligible(const cmbpo_mlp *m) {
  return m->head == CMBPO_HEAD_PROB && m->hidden == 512 && m->act == CMBPO_ACT_SWISH && m->o_tiles <= 4 && m->in_pad <= 64 &&
         2 * m->out_dim == m->o_width;
}

int cmbpo_internal_launch_h3(cmbpo_mlp *m, MlpKernelArgs &a, hipStream_t s) {
  if (m->h3_s0 == 0) {
    const int s0 = (m->in_pad + 15) / 16;
    m->h3_s0 = s0 < 2 ? 2 : s0;
    m->h3_otp = m->o_tiles <= 2 ? 2 : 4;
  }
  if (int rc = ensure_h3(m, s)) return rc;
  H3Args k{};
  k.m = a;
  const f16x8 *base = reinterpret_cast<const f16x8 *>(m->d_h3);
  k.w0 = base + m->h3_off[0]; k.w1 = base + m->h3_off[1]; k.w2 = base + m->h3_off[2];
  k.w0_stride = m->h3_stride[0]; k.w1_stride = m->h3_stride[1]; k.w2_stride = m->h3_stride[2];
  k.stats = reinterpret_cast<const float *>(reinterpret_cast<const char *>(m->d_h3) + m->h3_stats_off * 16);
  const int n_cu = cmbpo_cu_count();
  // Rows per item: the cheapest plan by a two-number model per item size -- the first round of a launch costs an item's
  // latency, every further round its steady-state time (tenths of a microsecond, measured by forcing each size over 17 row
  // counts, profiles/r03/h3_split_plan_sweep.log: 32 / 64 / 128 rows = 22.0 / 31.0 / 55.0 us then 17.5 / 30.0 / 54.0 us per
  // round at two output tiles; 25.5 / 36.0 / 72.0 then 19.8 / 34.3 / 70.5 at four -- Humanoid's 2 x 46 outputs take two
  // passes over the output layer, and 64-row items are its better main size).  The full rounds of one item size may be
  // followed by the leftovers at a SMALLER size in a launch of their own: a last round that would leave most CUs idle
  // becomes one or two rounds of short items on all of them (100 000 rows x 7 members = 5474 items of 128 rows on 256 CUs:
  // 21 full rounds + 98 items -> 196 items of 64 rows; 10 000 rows: 2 rounds of 128-row items + 41 items -> 164 of 32 rows,
  // 135 us by this model -- 134.5 measured -- against 147 for five rounds of 64-row items).  An item is (member, row tile) in
  // member-major order in every list, so a suffix of one list is a suffix of the others; a row's arithmetic does not depend
  // on the item it travels in (tests: bitwise against the forced sizes).
  // The main launch at 128 rows reads its x image from h3_ximage_kernel's blocks where that pays (g_h3_img_min_rows).
  const int E = m->ensemble;
  constexpr int kSplitGap = 40;     // the cost of the boundary between the two launches (tenths of a microsecond)
  int RT = g_h3_rt, RT_tail = 0, full = 0, tail_start = 0;
  if (RT == 0) {
    const int first_two[3] = {220, 310, 550}, steady_two[3] = {175, 300, 540};
    const int first_four[3] = {255, 360, 720}, steady_four[3] = {198, 343, 705};
    const int *first = m->h3_otp > 2 ? first_four : first_two, *steady = m->h3_otp > 2 ? steady_four : steady_two;
    const int rts[3] = {1, 2, 4};
    auto cost_of = [&](int i, long rounds) -> long { return rounds <= 0 ? 0 : first[i] + (rounds - 1) * steady[i]; };
    long best = -1;
    for (int i = 0; i < 3; ++i) {
      const long cost = cost_of(i, cmbpo_ceil_div(cmbpo_ceil_div(a.n_rows, 32 * rts[i]) * E, n_cu));
      if (best < 0 || cost <= best) { best = cost; RT = rts[i]; }
    }
    for (int i = 1; i < 3; ++i) {
      const int tiles_m = cmbpo_ceil_div(a.n_rows, 32 * rts[i]), n_m = tiles_m * E;
      const int fl = n_m / n_cu * n_cu, left = n_m - fl;
      if (fl == 0 || left == 0) continue;
      const int e0 = fl / tiles_m, t0 = fl - e0 * tiles_m;
      for (int j = 0; j < i; ++j) {
        const int tiles_t = cmbpo_ceil_div(a.n_rows, 32 * rts[j]);
        const int start = e0 * tiles_t + (rts[i] / rts[j]) * t0, n_tail = tiles_t * E - start;
        const long cost = cost_of(i, fl / n_cu) + cost_of(j, cmbpo_ceil_div(n_tail, n_cu)) + kSplitGap;
        if (cost < best) { best = cost; RT = rts[i]; RT_tail = rts[j]; full = fl; tail_start = start; }
      }
    }
  }
  const int S0 = m->h3_s0, OTP = m->h3_otp;
  // one launch: items [item0, end) of the (member-major) item list at rt 32-row tiles per item; end < 0: all of it
  // (the main launch of 128-row items on a stage-ahead instance reads the x image h3_ximage_kernel writes in front of it)
  auto launch = [&](int rt, int item0, int end, bool main) -> int {
    const int tiles = cmbpo_ceil_div(a.n_rows, 32 * rt);
    k.m.tiles = tiles;
    k.m.n_items = end < 0 ? tiles * E : end;     // (the kernel's loop bound)
    k.item0 = item0;
    const size_t lds = (size_t)lds_bytes(S0, rt);
    CMBPO_REQUIRE(lds <= 160 * 1024, "ens_h3: LDS budget exceeded (%zu B)", lds);
    const int n_here = k.m.n_items - item0;
    const int grid = n_here < n_cu ? n_here : n_cu;
    const bool img = main && rt == 4 && stage_ahead(S0, 4) && g_h3_img_min_rows >= 0 &&
                     (g_h3_img_min_rows == 0 ? n_here >= 2 * n_cu : a.n_rows >= g_h3_img_min_rows);
    k.ximg = nullptr;
    if (img) {
      if (int rc = ensure_ximg(m, a.n_rows, a.ld_rows, (size_t)ximg_block_bytes(S0))) return rc;
      k.ximg = reinterpret_cast<const char *>(m->d_ximg);
      if (S0 == 2) hipLaunchKernelGGL(h3_ximage_kernel<2>, dim3(tiles), dim3(kThreadsH), 0, s, k.m, reinterpret_cast<char *>(m->d_ximg));
      else hipLaunchKernelGGL(h3_ximage_kernel<3>, dim3(tiles), dim3(kThreadsH), 0, s, k.m, reinterpret_cast<char *>(m->d_ximg));
      CMBPO_HIP_CHECK(hipGetLastError());
    }
#define CMBPO_H3_CASE_I(S0_, OTP_, RT_, IMG_)                                                                          \
  if (S0 == S0_ && OTP == OTP_ && rt == RT_ && img == IMG_) {                                                          \
    if (int rc = cmbpo_grant_lds(ens_h3_kernel<S0_, OTP_, RT_, IMG_>, lds)) return rc;                                \
    hipLaunchKernelGGL((ens_h3_kernel<S0_, OTP_, RT_, IMG_>), dim3(grid), dim3(kThreadsH), lds, s, k);                \
  }
#define CMBPO_H3_CASE(S0_, OTP_, RT_) CMBPO_H3_CASE_I(S0_, OTP_, RT_, false)
#define CMBPO_H3_CASES(RT_)                                                                                            \
  CMBPO_H3_CASE(2, 2, RT_) CMBPO_H3_CASE(3, 2, RT_) CMBPO_H3_CASE(4, 2, RT_)                                           \
  CMBPO_H3_CASE(2, 4, RT_) CMBPO_H3_CASE(3, 4, RT_) CMBPO_H3_CASE(4, 4, RT_)
    CMBPO_H3_CASES(4) CMBPO_H3_CASES(2) CMBPO_H3_CASES(1)
    CMBPO_H3_CASE_I(2, 2, 4, true) CMBPO_H3_CASE_I(3, 2, 4, true) CMBPO_H3_CASE_I(2, 4, 4, true) CMBPO_H3_CASE_I(3, 4, 4, true)
#undef CMBPO_H3_CASES
#undef CMBPO_H3_CASE
#undef CMBPO_H3_CASE_I
    CMBPO_HIP_CHECK(hipGetLastError());
    return CMBPO_OK;
  };
  if (RT_tail) {
    if (int rc = launch(RT, 0, full, true)) return rc;
    return launch(RT_tail, tail_start, -1, false);
  }
  return launch(RT, 0, -1, true);
}

