// eval.hip -- the test loop's metrics (trainer.py:166-190) as integers that cross ranks exactly:
//
//   lbt_eval_tally   one launch per test batch: row[0] = the number of samples whose lowest-index maximum
//                    logit is the label (summary.hip's tie rule, argmax's), row[1] = the batch's loss-term
//                    sum in 2^-32 fixed point, bit for bit the loss_fx lbt_softmax_xent_n writes for the
//                    same (logits, labels). No dz, no loss: what a sharded test loop needs and no more.
//
// One workgroup, shaped as the softmax kernel whose sum it restates (xent_row.h holds the terms): classes
// <= 64 one thread per row (256 threads, rows t, t + 256, ...), wider heads one wave per row (16 waves,
// rows w, w + 16, ...). Latency-bound: a test batch's logits are a few KB to a few MB, read once.
#include "dfxp_device.h"
#include "xent_row.h"

using namespace lbt;

namespace {

__global__ __launch_bounds__(256) void eval_tally_kernel(const float* __restrict__ z,
                                                         const int32_t* __restrict__ labels, int N, int K,
                                                         long long* __restrict__ row) {
  __shared__ double red[256];
  __shared__ int cnt[256 / 64];
  double part = 0.0;
  int correct = 0;
  for (int r = threadIdx.x; r < N; r += 256) {
    const float* zr = z + (int64_t)r * K;
    float m, s;
    xent_row_stats(zr, K, m, s);
    const int y = labels[r];
    float best = zr[0];
    int idx = 0;
    for (int k = 1; k < K; ++k) {
      const float v = zr[k];
      if (v > best) {  // strict: the first maximum stays
        best = v;
        idx = k;
      }
    }
    correct += idx == y;
    // a label outside [0, K) names no logit: its row adds no loss term (and is never correct)
    if (y >= 0 && y < K) part += (double)xent_row_term(m, s, zr[y]);
  }
  const double total = xent_block_sum256(part, red);
  correct = wave_sum_i32(correct);
  if ((threadIdx.x & 63) == 0) cnt[threadIdx.x >> 6] = correct;
  __syncthreads();
  if (threadIdx.x == 0) {
    row[0] = (long long)(cnt[0] + cnt[1] + cnt[2] + cnt[3]);
    row[1] = xent_loss_fx(total);
  }
}

__global__ __launch_bounds__(1024) void eval_tally_wide_kernel(const float* __restrict__ z,
                                                               const int32_t* __restrict__ labels, int N, int K,
                                                               long long* __restrict__ row) {
  __shared__ double part[16];
  __shared__ int cnt[16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double acc = 0.0;
  int correct = 0;
  for (int rr = wave; rr < N; rr += 16) {
    const float* zr = z + (int64_t)rr * K;
    float m, s;
    xent_wave_stats(zr, K, lane, m, s);
    const int y = labels[rr];
    // a lane keeps its first maximum over k = lane, lane + 64, ...; the butterfly the lower index among
    // equal values (summary.hip's header_block)
    float best = -INFINITY;
    int idx = 0x7fffffff;
    if (lane < K) {
      best = zr[lane];
      idx = lane;
    }
    for (int k = lane + 64; k < K; k += 64) {
      const float v = zr[k];
      if (v > best) {
        best = v;
        idx = k;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(idx, o, 64);
      if (ov > best || (ov == best && oi < idx)) {
        best = ov;
        idx = oi;
      }
    }
    correct += idx == y;  // wave-uniform
    if (lane == 0 && y >= 0 && y < K) acc += (double)xent_row_term(m, s, zr[y]);
  }
  if (lane == 0) {
    part[wave] = acc;
    cnt[wave] = correct;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int c = 0;
    for (int w = 0; w < 16; ++w) c += cnt[w];
    row[0] = (long long)c;
    row[1] = xent_loss_fx(xent_wave_sum16(part));
  }
}

}  // namespace

extern "C" int lbt_eval_tally(const float* logits, const int32_t* labels, int32_t B, int32_t classes, int64_t* row,
                              void* stream) {
  if (!logits || !labels || !row || B <= 0 || classes < 1) return LBT_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (classes > 64)  // lbt_softmax_xent_n's split
    hipLaunchKernelGGL(eval_tally_wide_kernel, dim3(1), dim3(1024), 0, st, logits, labels, B, classes, (long long*)row);
  else
    hipLaunchKernelGGL(eval_tally_kernel, dim3(1), dim3(256), 0, st, logits, labels, B, classes, (long long*)row);
  return (int)hipGetLastError();
}
