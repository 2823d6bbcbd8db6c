// xent_row.h -- the per-row terms of the mean sparse softmax cross-entropy (models.py:30-32), shared by
// the kernels that must agree on them bit for bit: softmax_xent_kernel (misc.hip), the looped path of
// softmax_xent_wide_kernel (dense.hip) and eval_tally_kernel (eval.hip). A row's loss term is the float
// (logf(s) + m) - z[y] with m the row's maximum and s the fp32 sum of expf(z[k] - m) in the order each
// form fixes; the terms are added in double and leave the launch in 2^-32 fixed point.
#pragma once
#include "dfxp_device.h"

namespace lbt {

// One thread per row (K <= 64): the maximum and the sum over k ascending.
LBT_DEV void xent_row_stats(const float* __restrict__ zr, int K, float& m, float& s) {
  m = zr[0];
  for (int k = 1; k < K; ++k) m = zr[k] > m ? zr[k] : m;
  s = 0.f;
  for (int k = 0; k < K; ++k) s = s + expf(zr[k] - m);
}

// One wave per row (wide K): lane l takes k = l, l + 64, ... ascending, then the xor butterfly; every
// lane holds the row's m and s.
LBT_DEV void xent_wave_stats(const float* __restrict__ zr, int K, int lane, float& m, float& s) {
  m = -INFINITY;
  for (int k = lane; k < K; k += 64) m = fmaxf(m, zr[k]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  s = 0.f;
  for (int k = lane; k < K; k += 64) s = s + expf(zr[k] - m);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s = s + __shfl_xor(s, o, 64);
}

// The row's loss term from its statistics and the label's logit.
LBT_DEV float xent_row_term(float m, float s, float zy) {
  const float lse = logf(s) + m;
  return lse - zy;
}

// The block's ordered double sum as the exchange's loss slot carries it.
LBT_DEV long long xent_loss_fx(double t) { return (long long)llrint(t * 4294967296.0); }

// The narrow form's block sum: 256 per-thread partials (rows t, t + 256, ...) folded by halving strides.
// Every thread calls it; red[0] holds the sum afterwards (valid in thread 0 after the last barrier).
LBT_DEV double xent_block_sum256(double part, double* red) {
  red[threadIdx.x] = part;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}

// The wide form's block sum: the 16 wave partials (rows w, w + 16, ...) in wave order.
LBT_DEV double xent_wave_sum16(const double* part) {
  double t = 0.0;
  for (int w = 0; w < 16; ++w) t += part[w];
  return t;
}

}  // namespace lbt
