// bn_sync.hip -- SyncBN of the layer-wise models: a BatchNorm's sharded integer statistics folded to
// their totals, so that the collective which sums them over the ranks moves 1/32 of the bytes.
//   The layer-wise BN kernels take their moments from exact int64 channel sums [LBT_NSHARD][2C]
// (dynamic_fixed_point.py:588, tf.nn.moments over the whole batch) and their pass B from exact int64
// pass-A sums [LBT_NSHARD][4C] (:620-623). Summing either over the ranks before the kernel that
// consumes it makes N shards compute what one process computes on the whole batch; the fold writes
// the shard totals into shard 0 of a buffer whose other shards stay zero, which the unchanged
// consumers (sum_shards, bn_moments.h) read as they read any sharded buffer.
#include "dfxp_device.h"

using namespace lbt;

namespace {

// total[j] = sum_k part[k][j], j < stride: one thread per j, every shard's load in flight at once
// (sum_shards' loop, bn_moments.h). Launch-latency bound: at most 8192 outputs, 2 MiB read.
__global__ void sums_fold_kernel(const int64_t* __restrict__ part, int nshard, int64_t stride,
                                 int64_t* __restrict__ total) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= stride) return;
  long long v[LBT_NSHARD];
#pragma unroll
  for (int k = 0; k < LBT_NSHARD; ++k) v[k] = k < nshard ? part[(int64_t)k * stride + j] : 0;
  long long s = 0;
#pragma unroll
  for (int k = 0; k < LBT_NSHARD; ++k) s += v[k];
  total[j] = s;
}

}  // namespace

extern "C" int lbt_sums_fold(const int64_t* part, int32_t nshard, int64_t stride, int64_t* total, void* stream) {
  if (!part || !total || nshard <= 0 || nshard > LBT_NSHARD || stride <= 0) return LBT_EINVAL;
  hipLaunchKernelGGL(sums_fold_kernel, dim3((unsigned)((stride + 255) / 256)), dim3(256), 0, (hipStream_t)stream, part,
                     (int)nshard, stride, total);
  return (int)hipGetLastError();
}
