// The training loss of the ensembles, per element: what a kernel of the training step (ens_train.hip) or the training forward
// (ens_mlp.hip) needs to know about targets, weights, column kinds and the per-tile loss statistics.  Device code only.
#pragma once
#include "common.h"

// ------------------------------------------------------------------------------------------------------------
// The loss variants are compile-time modes.  A kernel that depends on the loss is a template over LossMode; its argument block
// is its base struct plus LossExtras<M> as a base class (WithLoss), so the plain instances have neither the pointers nor the
// code of the others and their argument block is the base struct, byte for byte.
//   LOSS_PLAIN  no extras
//   LOSS_VALUE  deterministic ('MSE') heads: per-sample weights and the clipped prediction of a trust-region value update,
//               pe.py:866-868,881-905,917
//   LOSS_COLW   probabilistic ('MSPE' / 'NLL') heads: column and class weights
//   LOSS_KINDS  probabilistic heads with logistic columns; always carries column weights (all ones from the
//               trainer's pool when none are attached)
// ------------------------------------------------------------------------------------------------------------
enum LossMode { LOSS_PLAIN, LOSS_VALUE, LOSS_COLW, LOSS_KINDS };
constexpr bool has_value(LossMode m) { return m == LOSS_VALUE; }
constexpr bool has_colw(LossMode m) { return m == LOSS_COLW || m == LOSS_KINDS; }
constexpr bool has_kinds(LossMode m) { return m == LOSS_KINDS; }

struct ValueExtras {
  const float *w;          // [N] weight of data row r (nullptr: 1)
  const float *old_pred;   // [N][D] earlier prediction of row r, unscaled (nullptr: no clipping)
  const float *clip_c;     // the step's clip range c = sqrt(2) sqrt(kl old_var) (old_var_final_kernel); read when old_pred is set
};
// Element (row, d) of a member's batch weighs col[d], times pos[d] where the RAW target (before the output scaler) is positive
// (the definition stands in include/cmbpo_hip.h).
struct ColWeights {
  const float *col, *pos;  // [D] each, both set
};

template <LossMode M> struct LossExtras {};
template <> struct LossExtras<LOSS_VALUE> : ValueExtras {};
template <> struct LossExtras<LOSS_COLW> : ColWeights {};
template <> struct LossExtras<LOSS_KINDS> : ColWeights {
  const unsigned char *kind;   // [D]; kind[d] != 0: column d is logistic (cmbpo_trainer_set_column_kinds)
};
template <class Base, LossMode M> struct WithLoss : Base, LossExtras<M> {};

// ------------------------------------------------------------------------------------------------------------
// Targets: row through the member's index list, raw target, target through the output scaler
// ------------------------------------------------------------------------------------------------------------
struct TargetView {
  const float *targets;    // [N][D]
  const int32_t *idx;      // [E][idx_stride] rows of `targets` (nullptr: row b)
  int idx_stride;
  const float *out_mu, *out_sig;   // output scaler (nullptr: identity)
  int D;
  __device__ __forceinline__ int src_row(int e, int b) const { return idx ? idx[(size_t)e * idx_stride + b] : b; }
  __device__ __forceinline__ float raw(int src, int d) const { return targets[(size_t)src * D + d]; }
  // TensorStandardScaler.transform, models/pens/utils.py:156; also takes an old prediction to the targets' unit
  __device__ __forceinline__ float scaled(float v, int d) const {
    if (out_mu) v = (v - out_mu[d]) / out_sig[d];
    return v;
  }
};
// of an argument block that names its fields as the view does
template <class A>
__device__ __forceinline__ TargetView target_view(const A &p) {
  return TargetView{p.targets, p.idx, p.idx_stride, p.out_mu, p.out_sig, p.D};
}

// ------------------------------------------------------------------------------------------------------------
// Per-element terms
// ------------------------------------------------------------------------------------------------------------
// The test is written positively: a NaN target takes the plain weight.
__device__ __forceinline__ float column_weight(const ColWeights &c, int d, float raw_target) {
  return c.col[d] * (raw_target > 0.5f ? c.pos[d] : 1.0f);
}

// The weight of element (src, d) on every data term of its loss.  The literal 1.0f of the plain mode folds away exactly
// (the build runs with -ffp-contract=off and without fast-math: 1.0f * x is x).
template <LossMode M>
__device__ __forceinline__ float loss_weight(const LossExtras<M> &x, int src, int d, float raw_target) {
  if constexpr (has_value(M)) return x.w ? x.w[src] : 1.0f;
  else if constexpr (has_colw(M)) return column_weight(x, d, raw_target);
  else return 1.0f;
}

// (m_c - t') w of one output, with the gradient of tf.clip_by_value: nothing outside [-c, c].  olds is the scaled old prediction.
__device__ __forceinline__ float value_delta(float m, float t, bool clip, float olds, float c, float w) {
  float d = m - t;
  if (clip) {
    const float dm = m - olds;
    const float mc = olds + fminf(fmaxf(dm, -c), c);
    d = (dm >= -c && dm <= c) ? mc - t : 0.0f;
  }
  return w * d;
}
// the old prediction in the unit of the scaled targets: both sides of the clip in one unit
__device__ __forceinline__ float scaled_old(const ValueExtras &x, const TargetView &tv, int src, int d) {
  return tv.scaled(x.old_pred[(size_t)src * tv.D + d], d);
}

// A logistic column reads its mean output as a logit z and trains it with the Bernoulli negative log-likelihood of y = (raw
// target > 0.5f), never through the output scaler.
__device__ __forceinline__ float bernoulli_nll(float z, bool y) {     // softplus(z) - y z, finite for every finite z
  return fmaxf(z, 0.0f) - (y ? z : 0.0f) + log1pf(expf(-fabsf(z)));
}
__device__ __forceinline__ float sigmoid_of(float z) {
  if (z >= 0.0f) return 1.0f / (1.0f + expf(-z));
  const float ez = expf(z);
  return ez / (1.0f + ez);
}

// ------------------------------------------------------------------------------------------------------------
// The loss statistics of one tile of ROWS rows of a member on NT threads: sum w (m - t)^2, sum w (var - mse)^2, sum lv^2 (the
// last two with `prob` only; logistic columns stay out of the first two and in the third).  out(b, k) is raw output k of tile
// row b, src_row(b) its row of the targets (< 0: past the batch).  The backward kernel adds the tiles' sums in a fixed order
// (mspe_ratio), so the step needs no reduction kernel and no atomics.  Whoever computes a tile's statistics -- the training
// forwards in mode LOSS_PLAIN, col_stats_kernel over their stored outputs in the weighted modes -- computes them here: one
// element-to-thread map, one set of float32 terms, one order of the float64 sums, so all-ones weights give the plain bits.
// Contains a barrier: the whole workgroup calls it.  Returns statistic `tid` of the tile in threads 0..2.
// ------------------------------------------------------------------------------------------------------------
template <int ROWS, int NT, LossMode M, class Out, class Src>
__device__ __forceinline__ double tile_loss_stats(const TargetView &tv, const LossExtras<M> &x, bool prob, int wave, Out out, Src src_row) {
  constexpr int NW = NT / 64;
  const int tid = threadIdx.x, lane = tid & 63;
  const int D = tv.D;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (int i = tid; i < ROWS * D; i += NT) {
    const int b = i / D, d = i - b * D;
    const int src = src_row(b);
    if (src < 0) continue;
    const float traw = tv.raw(src, d), t = tv.scaled(traw, d);
    if constexpr (has_kinds(M)) {
      if (x.kind[d]) { const float lv = out(b, D + d); s2 += (double)(lv * lv); continue; }
    }
    const float diff = out(b, d) - t;
    const float mse = diff * diff;
    const float w = loss_weight<M>(x, src, d, traw);
    s0 += (double)(w * mse);
    if (prob) {
      const float lv = out(b, D + d);
      const float dv = expf(lv) - mse;
      s1 += (double)(w * (dv * dv));
      s2 += (double)(lv * lv);
    }
  }
  __shared__ double s_loss[3][NW];
  s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2);
  if (lane == 0) { s_loss[0][wave] = s0; s_loss[1][wave] = s1; s_loss[2][wave] = s2; }
  __syncthreads();
  double tsum = 0.0;
  if (tid < 3) {
    if constexpr (NW == 4) tsum = (s_loss[tid][0] + s_loss[tid][1]) + (s_loss[tid][2] + s_loss[tid][3]);
    else
      for (int w = 0; w < NW; ++w) tsum += s_loss[tid][w];
  }
  return tsum;
}

// A tile's statistics into the [items][3] array, by threads 0..2.  A 64-row item's sums stand in the first of its two 32-row
// slots (the backward kernel adds the entries of all 32-row tiles); zero_next clears the second.
__device__ __forceinline__ void store_tile_stats(double *loss_part, size_t item, bool zero_next, double v) {
  if (threadIdx.x < 3) {
    loss_part[item * 3 + threadIdx.x] = v;
    if (zero_next) loss_part[(item + 1) * 3 + threadIdx.x] = 0.0;
  }
}
