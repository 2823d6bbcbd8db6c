// summary.hip -- the reference's training summaries (tf.summary.scalar of every *_range and parameter
// mean, dynamic_fixed_point.py:180-190 ..., fetched with loss and accuracy, trainer.py:148-155) recorded
// on the device inside a captured step:
//
//   lbt_summary_record   after the backward, before the update: the step counter, every quantiser's
//                        range, overflow-counter totals and element count, every parameter tensor's
//                        double sum (per-chunk partials), and the batch's correct-prediction count
//   lbt_summary_commit   after the update: folds the chunk partials, copies the loss, advances the cursor
//
// Both write ring slot cursor[0] % capacity (record layout: include/lbt_dfxp.h). Every source is read
// only. One launch each; the record launch's workgroups are [parameter chunks | 4 slots each | 1 header +
// accuracy]. Latency-bound at ResNet-20's 272 K parameters, a streaming read at ResNet-50's 25 M.
#include "dfxp_device.h"

using namespace lbt;

namespace {

constexpr int kT = 256;
constexpr int64_t kChunk = LBT_SUMMARY_CHUNK;
constexpr int64_t kHeader = 32;

LBT_DEV int64_t rec_bytes(int nslots, int nparams) { return kHeader + 16 * (int64_t)nslots + 8 * (int64_t)nparams; }
LBT_DEV uint8_t* rec_base(const lbt_summary& s) {
  const uint64_t slot = s.cursor[0] % (uint64_t)s.capacity;
  return static_cast<uint8_t*>(s.ring) + (int64_t)slot * rec_bytes(s.nslots, s.nparams);
}
LBT_DEV double* rec_sums(const lbt_summary& s, uint8_t* rec) {
  return reinterpret_cast<double*>(rec + kHeader + 16 * (int64_t)s.nslots);
}

LBT_DEV double wave_sum_f64(double v) {  // a fixed butterfly: the same bits in every lane, every run
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One chunk of one parameter segment: thread t adds float4 t, t + 256, ... (one accumulator per
// component), the up-to-3 head elements in front of the first 16-byte boundary and the up-to-3 tail
// elements behind the last whole float4 go to threads 0..2; wave butterflies, then the four wave totals
// in order. fp32 -> double is exact, and every association is fixed by (address mod 16, length).
LBT_DEV void param_block(const lbt_summary& s, int blk, int cps, double* sh) {
  const int p = blk / cps, chunk = blk - p * cps;
  const int64_t b0 = s.seg_off[p], b1 = s.seg_off[p + 1];
  int64_t start = b0 + (int64_t)chunk * kChunk, end = start + kChunk;
  if (end > b1) end = b1;
  const int t = threadIdx.x;
  double acc = 0.0;
  if (start < end) {  // (an empty chunk stores 0.0)
    const float* __restrict__ x = s.w + start;
    const int64_t n = end - start;
    int64_t head = (int64_t)((4u - (unsigned)((reinterpret_cast<uintptr_t>(x) >> 2) & 3u)) & 3u);
    if (head > n) head = n;
    if (t < head) acc = (double)x[t];
    const float4* __restrict__ x4 = reinterpret_cast<const float4*>(x + head);
    const int64_t n4 = (n - head) >> 2;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (int64_t i = t; i < n4; i += kT) {
      const float4 v = x4[i];
      a0 += (double)v.x;
      a1 += (double)v.y;
      a2 += (double)v.z;
      a3 += (double)v.w;
    }
    acc += (a0 + a1) + (a2 + a3);
    const int64_t tail = head + 4 * n4 + t;
    if (t < 3 && tail < n) acc += (double)x[tail];
  }
  acc = wave_sum_f64(acc);
  if ((t & 63) == 0) sh[t >> 6] = acc;
  __syncthreads();
  if (t == 0) s.scratch[blk] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// One wave per slot: lane k < LBT_NSHARD reads shard k (wave_shard_totals without its stores).
LBT_DEV void slot_wave(const lbt_summary& s, int i, uint8_t* rec) {
  const int lane = threadIdx.x & 63;
  int a = 0, b = 0;
  if (lane < LBT_NSHARD) {
    const int32_t* c = s.counts + ((int64_t)i * LBT_NSHARD + lane) * LBT_CSTRIDE;
    a = c[0];
    b = c[1];
  }
  const int c1 = wave_sum_i32(a), c2 = wave_sum_i32(b);
  if (lane == 0) {
    int32_t* o = reinterpret_cast<int32_t*>(rec + kHeader);
    const int64_t ns = s.nslots;
    o[i] = s.exps[i];
    o[ns + i] = c1;
    o[2 * ns + i] = c2;
    reinterpret_cast<float*>(o)[3 * ns + i] = s.nelem[i];
  }
}

// The header and the accuracy count: wave w takes samples w, w + 4, ...; a lane scans classes lane,
// lane + 64, ... keeping its first maximum, the butterfly keeps the lower index among equal values.
LBT_DEV void header_block(const lbt_summary& s, uint8_t* rec, int* sh) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int correct = 0;
  for (int b = wv; b < s.batch; b += kT / 64) {
    const float* __restrict__ z = s.logits + (int64_t)b * s.classes;
    float best = -INFINITY;
    int idx = 0x7fffffff;
    if (lane < s.classes) {
      best = z[lane];
      idx = lane;
    }
    for (int j = lane + 64; j < s.classes; j += 64) {
      const float v = z[j];
      if (v > best) {
        best = v;
        idx = j;
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
    correct += idx == s.labels[b];  // wave-uniform
  }
  if (lane == 0) sh[wv] = correct;
  __syncthreads();
  if (threadIdx.x == 0) {
    *reinterpret_cast<uint64_t*>(rec) = s.step[0];
    int32_t* h = reinterpret_cast<int32_t*>(rec);
    h[2] = s.batch;
    h[3] = sh[0] + sh[1] + sh[2] + sh[3];
    h[5] = s.nslots;
    h[6] = s.nparams;
    h[7] = 0;
  }
}

__global__ __launch_bounds__(kT) void summary_record_kernel(const lbt_summary s, int pblocks, int cps, int sblocks) {
  __shared__ double shd[kT / 64];
  __shared__ int shi[kT / 64];
  const int blk = blockIdx.x;
  if (blk < pblocks) {
    param_block(s, blk, cps, shd);
    return;
  }
  uint8_t* rec = rec_base(s);
  if (blk < pblocks + sblocks) {
    const int i = (blk - pblocks) * (kT / 64) + (int)(threadIdx.x >> 6);
    if (i < s.nslots) slot_wave(s, i, rec);
    return;
  }
  header_block(s, rec, shi);
}

// One workgroup: every thread reads the cursor before the barrier, thread 0 advances it behind it.
__global__ __launch_bounds__(kT) void summary_commit_kernel(const lbt_summary s, int cps) {
  const uint64_t cur = s.cursor[0];
  uint8_t* rec = static_cast<uint8_t*>(s.ring) + (int64_t)(cur % (uint64_t)s.capacity) * rec_bytes(s.nslots, s.nparams);
  double* sums = rec_sums(s, rec);
  for (int p = threadIdx.x; p < s.nparams; p += kT) {
    const double* part = s.scratch + (int64_t)p * cps;
    double t = part[0];
    for (int c = 1; c < cps; ++c) t += part[c];
    sums[p] = t;
  }
  if (threadIdx.x == 0) reinterpret_cast<float*>(rec)[4] = s.loss[0];
  __syncthreads();
  if (threadIdx.x == 0) s.cursor[0] = cur + 1ull;
}

int64_t chunks_per_seg(int64_t max_seg) { return max_seg > 0 ? (max_seg + kChunk - 1) / kChunk : 1; }

// the argument checks of both entry points (host only); the record launch's grid on success
struct Grid { int pblocks, cps, sblocks; };
int check(const lbt_summary* s, Grid* g) {
  if (!s) return LBT_EINVAL;
  if (s->capacity <= 0 || s->nslots < 0 || s->nparams < 0 || s->batch < 0 || s->classes < 1) return LBT_EINVAL;
  if (!s->ring || !s->cursor || !s->step) return LBT_EINVAL;
  if (s->nslots > 0 && (!s->exps || !s->counts || !s->nelem)) return LBT_EINVAL;
  if (s->nparams > 0 && (!s->w || !s->seg_off || !s->scratch || s->max_seg <= 0)) return LBT_EINVAL;
  if (s->batch > 0 && (!s->logits || !s->labels)) return LBT_EINVAL;
  const int64_t lim = (int64_t)1 << 31;
  const int64_t cps = s->nparams > 0 ? chunks_per_seg(s->max_seg) : 1;
  if (cps >= lim) return LBT_EINVAL;
  const int64_t pblocks = (int64_t)s->nparams * cps, sblocks = ((int64_t)s->nslots + 3) / 4;
  if (pblocks + sblocks + 1 >= lim) return LBT_EINVAL;
  *g = Grid{(int)pblocks, (int)cps, (int)sblocks};
  return LBT_OK;
}

}  // namespace

extern "C" int64_t lbt_summary_record_bytes(int32_t nslots, int32_t nparams) {
  if (nslots < 0 || nparams < 0) return -LBT_EINVAL;
  return kHeader + 16 * (int64_t)nslots + 8 * (int64_t)nparams;
}

extern "C" int64_t lbt_summary_scratch_bytes(int32_t nparams, int64_t max_seg) {
  if (nparams < 0 || max_seg < 0) return -LBT_EINVAL;
  return 8 * (int64_t)nparams * chunks_per_seg(max_seg);
}

extern "C" int lbt_summary_record(const lbt_summary* s, void* stream) {
  Grid g;
  const int rc = check(s, &g);
  if (rc) return rc;
  hipLaunchKernelGGL(summary_record_kernel, dim3((unsigned)(g.pblocks + g.sblocks + 1)), dim3(kT), 0,
                     (hipStream_t)stream, *s, g.pblocks, g.cps, g.sblocks);
  return (int)hipGetLastError();
}

extern "C" int lbt_summary_commit(const lbt_summary* s, void* stream) {
  Grid g;
  const int rc = check(s, &g);
  if (rc) return rc;
  if (!s->loss) return LBT_EINVAL;
  hipLaunchKernelGGL(summary_commit_kernel, dim3(1), dim3(kT), 0, (hipStream_t)stream, *s, g.cps);
  return (int)hipGetLastError();
}
