// What the two policy-update kernels -- pi_kernel (fp32 MFMAs, policy_update.hip) and pi_kernel_h (three-term f16,
// pi_kernel_f16.h) -- share outside their matrix products: the first-order gate and coefficients at entry, the one-time LDS
// set-up, the per-sample formulas of the surrogate and the KL, and the flush of the loss sums.
// Included by policy_update.hip inside its anonymous namespace, after PiArgs; device code only.
// The kernels keep every __shared__ declaration and hand pointers in (a declaration in here moves the static LDS layout),
// and they keep the loss accumulators as scalars of their own (gathered in a struct, the f16 first-order kernels are
// allocated differently).  DESIGN, "Where the policy-update math lives", says what stays per kernel and why.
#pragma once

// the per-sample weight of the clipped, penalised surrogate's cotangent, and what the sample adds to the objective:
//   min_adv = adv > 0 ? (1 + clip) adv : (1 - clip) adv;  active = !clipped || ratio adv <= min_adv   (positive test: a NaN
//   ratio is inactive; on a tie the first argument of the minimum is the active one, as in tf.minimum)
//   w = -c_r (active ? adv : 0) + c_c cadv
__device__ __forceinline__ float ppo_weight(float ratio, float adv, float cadv, float clip, bool clipped, float c_r, float c_c,
                                            float &obj, bool &active) {
  const float ra = ratio * adv;
  const float min_adv = adv > 0.0f ? (1.0f + clip) * adv : (1.0f - clip) * adv;
  active = !clipped || (ra <= min_adv);
  obj = active ? ra : min_adv;
  return -c_r * (active ? adv : 0.0f) + c_c * cadv;
}

// MODE_PPO with weights: this lane's share of the weights of the workgroup's tiles (a second walk over them, behind the tile
// loop, where it costs no register: the rows can be counted from the tile walk, their weights cannot)
__device__ __forceinline__ double tile_walk_weights(const float *wt, int n, int n_tiles, int lane) {
  double s = 0.0;
  for (int t = blockIdx.x + (lane >> 5) * gridDim.x; t < n_tiles; t += 2 * gridDim.x) {
    const int r = t * BB + (lane & 31);
    if (r < n) s += (double)wt[r];
  }
  return s;
}

// one (sample, action) term of gaussian_kl(mu, log_std, mu_old, log_std_old), ac_network.py:50-55; dm = mu_old - mu
__device__ __forceinline__ float gauss_kl_term(float dm, float ls, float lso) {
  return 0.5f * ((dm * dm + expf(2.0f * ls)) / (expf(2.0f * lso) + 1e-8f) - 1.0f) + lso - ls;
}

// ---- entry -------------------------------------------------------------------------------------------------------------------
// MODE_PPO: the first-order loop's gate has stopped this pass (uniform: one scalar load, one branch)
template <int MODE>
__device__ __forceinline__ bool pi_ppo_stopped(const PiArgs &p) {
  if constexpr (MODE == MODE_PPO) return (p.ppo_flags & PPO_GATED) && p.state[ST_STOP] != 0.0;
  return false;
}
// the penalty's coefficients c_r, c_c (1, 0 unless MODE_PPO runs the penalised objective)
template <int MODE>
__device__ __forceinline__ void pi_ppo_coeffs(const PiArgs &p, float &c_r, float &c_c) {
  c_r = 1.0f;
  c_c = 0.0f;
  if constexpr (MODE == MODE_PPO) {
    if (p.ppo_flags & PPO_PENALIZED) {
      c_r = (float)p.state[ST_CR];
      c_c = (float)p.state[ST_CC];
    }
  }
}

// zero the padded cotangent columns (a in [A, 36)) and the padded input columns (k in [D, XS)) once: nothing else ever writes
// them.  NTHR threads.
template <int NTHR>
__device__ __forceinline__ void pi_zero_pads(float *wR, float *xR, int XS, int tid) {
  for (int i = tid; i < BB * 36; i += NTHR) wR[i] = 0.0f;
  for (int i = tid; i < BB * XS; i += NTHR) xR[i] = 0.0f;
  __syncthreads();
}

// Fisher cotangent: its tile-invariant factors per action column, computed once (LDS: no registers to spare)
template <int MODE>
__device__ __forceinline__ void pi_fisher_consts(const PiArgs &p, const PiDims &d, float *c_b2, float *c_e2, int tid) {
  if constexpr (MODE == MODE_FVP) {
    if (tid < 32) {
      c_b2[tid] = (tid < d.A) ? p.v.b2[tid] : 0.0f;
      c_e2[tid] = (tid < d.A) ? 2.0f * expf(2.0f * p.w.ls[tid]) : 0.0f;
    }
    __syncthreads();
  }
}

// ---- flush of the loss sums ----------------------------------------------------------------------------------------------------
// MODE_EVAL, MODE_GRAD: float64 atomics; MODE_PPO: the workgroup's ordered partials, with its row count or, WT, the weights of
// its rows.  Threads tid < 32 hold the per-sample sums, s_kl is spread over every thread; sd: [NW] doubles of LDS, NW waves.
template <int MODE, bool WT, int NW>
__device__ __forceinline__ void pi_flush_sums(const PiArgs &p, double *sd, int n_tiles, int lane, int wave, double s_n, double s_ra,
                                              double s_rc, double s_kl, double s_cost, double s_obj, int s_nclip, float s_clipw) {
  const double kl = wave_sum(s_kl);
  if (lane == 0) sd[wave] = kl;
  __syncthreads();
  if (wave == 0) {
    const double n = wave_sum(s_n), ra = wave_sum(s_ra), rc = wave_sum(s_rc), c = wave_sum(s_cost);
    if constexpr (MODE == MODE_PPO) {
      const double ob = wave_sum(s_obj), nc = wave_sum(WT ? (double)s_clipw : (double)s_nclip);
      const double wsum = WT ? wave_sum(tile_walk_weights(p.wt, p.n, n_tiles, lane)) : 0.0;
      if (lane == 0) {
        double klt = sd[0];
#pragma unroll
        for (int wv = 1; wv < NW; ++wv) klt += sd[wv];
        double *sp = p.sums_part + (size_t)blockIdx.x * 8;
        int rows = 0;
        if constexpr (!WT)
          for (int t = blockIdx.x; t < n_tiles; t += gridDim.x) rows += min(BB, p.n - t * BB);
        sp[0] = WT ? wsum : (double)rows; sp[1] = ob; sp[2] = rc; sp[3] = klt; sp[4] = c; sp[5] = nc; sp[6] = ra; sp[7] = 0.0;
      }
    } else if (lane == 0) {
      atomicAdd(&p.sums[0], n);
      atomicAdd(&p.sums[1], ra);
      atomicAdd(&p.sums[2], rc);
      double klt = sd[0];
#pragma unroll
      for (int wv = 1; wv < NW; ++wv) klt += sd[wv];
      atomicAdd(&p.sums[3], klt);
      atomicAdd(&p.sums[4], c);
    }
  }
}
