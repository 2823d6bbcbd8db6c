// dropout.hip -- Dropout_q (dynamic_fixed_point.py:1025-1040, tf.nn.dropout) for gfx950.
//
//  lbt_dropout_fwd       y  = fl32(x / keep) * mask, optionally on max(x, 0)
//  lbt_dropout_bwd       dx = fl32(g / keep) * mask, the mask regenerated from its counter
//  lbt_dropout_quantize  dropout + the next layer's input quantiser in one pass: 4 B in, 1-2 B out
//  lbt_dropout_*_at      the same three on a window of the stream: local element i draws the mask of
//                        element base + i (a rank's shard of the global batch); the plain entry points
//                        are base = 0
//
// The mask of element i of the whole tensor (batch included: tf.nn.dropout draws x.shape noise) is
//   u_i = Philox4x32-10((i >> 2, did, step_lo, step_hi), (seed_lo, seed_hi))[i & 3] >> 8, times 2^-24
//   m_i = fl32(keep + u_i) >= 1
// on the Philox stream of the quantisers (dfxp_device.h), keyed by the layer's id `did` where they
// use their range variable's. One thread owns four consecutive elements: one Philox call, one
// 16-byte load and one store. All three are HBM-bound streaming passes. A base that is no multiple
// of 4 puts a thread's four elements across two Philox blocks: those launches take the per-element
// kernels (one Philox call per element).
#include "dfxp_device.h"

using namespace lbt;

namespace {

constexpr int kThreads = 256;
constexpr int64_t kMaxN = (int64_t)1 << 34;  // the Philox block counter i >> 2 is 32 bits

// One element: the correctly rounded fp32 quotient, then an fp32 multiply by the 0 / 1 mask (a
// dropped element is that product: -0.0 for a negative x, NaN for a non-finite one, as in TF).
LBT_DEV float drop1(float x, float keep, float u, int relu) {
  if (relu) x = x > 0.f ? x : 0.f;
  const float m = (keep + u) >= 1.0f ? 1.0f : 0.0f;
  return (x / keep) * m;
}

__global__ __launch_bounds__(kThreads) void dropout_fwd_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                               int64_t n, float keep, const uint64_t* __restrict__ step,
                                                               uint64_t seed, uint32_t did, int relu, int vec,
                                                               int64_t blk0) {
  const int64_t blk = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int64_t i = blk << 2;
  if (i >= n) return;
  const Noise4 u = noise4((uint64_t)(blk0 + blk), did, step[0], seed);  // blk0 = base / 4
  if (vec && i + 4 <= n) {
    const float4 v = *reinterpret_cast<const float4*>(x + i);
    float4 o;
    o.x = drop1(v.x, keep, u.u[0], relu); o.y = drop1(v.y, keep, u.u[1], relu);
    o.z = drop1(v.z, keep, u.u[2], relu); o.w = drop1(v.w, keep, u.u[3], relu);
    *reinterpret_cast<float4*>(y + i) = o;
  } else {  // the tail of n % 4 != 0, or buffers that are not 16-byte aligned
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (i + k < n) y[i + k] = drop1(x[i + k], keep, u.u[k], relu);
  }
}

// base % 4 != 0: one element per thread, its own Philox call at the global index base + i
__global__ __launch_bounds__(kThreads) void dropout_fwd_elem_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                    int64_t n, float keep,
                                                                    const uint64_t* __restrict__ step, uint64_t seed,
                                                                    uint32_t did, int relu, int64_t base) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  y[i] = drop1(x[i], keep, noise1((uint64_t)(base + i), did, step[0], seed), relu);
}

// relu_x: the input of a ReLU folded in front (lbt_dropout_fwd's relu = 1) -- its mask on top, as
// relu_bwd_kernel applies it (g where x > 0, else +0)
LBT_DEV float drop_bwd1(float g, float keep, float u, bool has_rx, float rx) {
  const float d = drop1(g, keep, u, 0);
  return has_rx ? (rx > 0.f ? d : 0.f) : d;
}

__global__ __launch_bounds__(kThreads) void dropout_bwd_kernel(const float* __restrict__ g, float* __restrict__ dx,
                                                               int64_t n, float keep, const uint64_t* __restrict__ step,
                                                               uint64_t seed, uint32_t did,
                                                               const float* __restrict__ relu_x, int vec,
                                                               int64_t blk0) {
  const int64_t blk = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int64_t i = blk << 2;
  if (i >= n) return;
  const Noise4 u = noise4((uint64_t)(blk0 + blk), did, step[0], seed);
  const bool rx = relu_x != nullptr;
  if (vec && i + 4 <= n) {
    const float4 v = *reinterpret_cast<const float4*>(g + i);
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (rx) r = *reinterpret_cast<const float4*>(relu_x + i);
    float4 o;
    o.x = drop_bwd1(v.x, keep, u.u[0], rx, r.x); o.y = drop_bwd1(v.y, keep, u.u[1], rx, r.y);
    o.z = drop_bwd1(v.z, keep, u.u[2], rx, r.z); o.w = drop_bwd1(v.w, keep, u.u[3], rx, r.w);
    *reinterpret_cast<float4*>(dx + i) = o;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (i + k < n) dx[i + k] = drop_bwd1(g[i + k], keep, u.u[k], rx, rx ? relu_x[i + k] : 0.f);
  }
}

__global__ __launch_bounds__(kThreads) void dropout_bwd_elem_kernel(const float* __restrict__ g, float* __restrict__ dx,
                                                                    int64_t n, float keep,
                                                                    const uint64_t* __restrict__ step, uint64_t seed,
                                                                    uint32_t did, const float* __restrict__ relu_x,
                                                                    int64_t base) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const bool rx = relu_x != nullptr;
  dx[i] = drop_bwd1(g[i], keep, noise1((uint64_t)(base + i), did, step[0], seed), rx, rx ? relu_x[i] : 0.f);
}

// quantize_rows_kernel (quantize.hip) with dropout applied to each element on its way in: the same
// grid, rows per thread, counter reduction and shard per workgroup, so the codes AND every counter
// shard equal lbt_dropout_fwd followed by lbt_dfxp_quantize. The quantiser's noise is per column
// group (index mod inner: once per thread), the dropout's per element of the whole tensor (one
// Philox call per row: inner % 4 == 0 and gbase % 4 == 0 keep a thread's four elements inside one
// Philox block). gbase: the global index of local element 0.
__global__ __launch_bounds__(kThreads) void dropout_quantize_rows_kernel(
    const float* __restrict__ x, void* __restrict__ out, int out_kind, int64_t rows, int64_t inner, int rpt,
    float keep, uint32_t did, int relu, lbt_qdesc q, int64_t gbase) {
  __shared__ int sh_cnt[2 * kThreads / 64];
  const QState s = qstate(q);
  const int64_t groups = inner >> 2;
  const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.y * rpt;
  int ov1 = 0, ov2 = 0;
  if (g < groups) {
    Noise4 n = {{0.f, 0.f, 0.f, 0.f}};
    if (q.stochastic) n = qnoise4(q, s.step, g);
    const int64_t rend = r0 + rpt < rows ? r0 + rpt : rows;
#pragma unroll 4
    for (int64_t r = r0; r < rend; ++r) {
      const int64_t base = r * inner + (g << 2);
      const float4 v = *reinterpret_cast<const float4*>(x + base);
      const Noise4 u = noise4((uint64_t)((gbase + base) >> 2), did, s.step, q.seed);
      int c[4];
      c[0] = quant1(s, q.stochastic, drop1(v.x, keep, u.u[0], relu), n.u[0], ov1, ov2);
      c[1] = quant1(s, q.stochastic, drop1(v.y, keep, u.u[1], relu), n.u[1], ov1, ov2);
      c[2] = quant1(s, q.stochastic, drop1(v.z, keep, u.u[2], relu), n.u[2], ov1, ov2);
      c[3] = quant1(s, q.stochastic, drop1(v.w, keep, u.u[3], relu), n.u[3], ov1, ov2);
      if (out_kind == LBT_OUT_I16) {
        short4 o;
        o.x = (short)c[0]; o.y = (short)c[1]; o.z = (short)c[2]; o.w = (short)c[3];
        *reinterpret_cast<short4*>((int16_t*)out + base) = o;
      } else {
        const int off = out_kind == LBT_OUT_U8OFF ? 128 : 0;
        char4 o;
        o.x = (int8_t)((out_kind == LBT_OUT_U8OFF && c[0] < 0 ? 0 : c[0]) - off);
        o.y = (int8_t)((out_kind == LBT_OUT_U8OFF && c[1] < 0 ? 0 : c[1]) - off);
        o.z = (int8_t)((out_kind == LBT_OUT_U8OFF && c[2] < 0 ? 0 : c[2]) - off);
        o.w = (int8_t)((out_kind == LBT_OUT_U8OFF && c[3] < 0 ? 0 : c[3]) - off);
        *reinterpret_cast<char4*>((int8_t*)out + base) = o;
      }
    }
  }
  if (!q.counts) return;  // uniform
  counts_stage(0, 1, ov1, ov2, sh_cnt);
  __syncthreads();
  counts_publish(0, 1, q, sh_cnt);
}

// Any shape (quantize_generic_kernel's grid): one element per thread, per-element Philox for both.
__global__ __launch_bounds__(kThreads) void dropout_quantize_generic_kernel(
    const float* __restrict__ x, void* __restrict__ out, int out_kind, int64_t n, int64_t inner, float keep,
    uint32_t did, int relu, lbt_qdesc q, int64_t gbase) {
  __shared__ int sh_cnt[2 * kThreads / 64];
  const QState s = qstate(q);
  int ov1 = 0, ov2 = 0;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    const float ud = noise1((uint64_t)(gbase + i), did, s.step, q.seed);
    const float u = q.stochastic ? qnoise1(q, s.step, i % inner) : 0.f;
    const int c = quant1(s, q.stochastic, drop1(x[i], keep, ud, relu), u, ov1, ov2);
    store_code(out, out_kind, i, c, s.inv_m);
  }
  block_flush_counts(q, ov1, ov2, sh_cnt);
}

bool keep_ok(float keep) { return keep > 0.f && keep <= 1.f; }  // false for NaN
// the window [base, base + n) lies inside the stream's 2^34 elements
bool window_ok(int64_t base, int64_t n) { return n >= 0 && base >= 0 && n <= kMaxN && base <= kMaxN - n; }

}  // namespace

extern "C" int lbt_dropout_fwd_at(const float* x, float* y, int64_t n, int64_t base, float keep, const uint64_t* step,
                                  uint64_t seed, uint32_t did, int32_t relu, void* stream) {
  if (!window_ok(base, n) || !keep_ok(keep) || !step) return LBT_EINVAL;
  if (n == 0) return LBT_OK;
  hipStream_t st = (hipStream_t)stream;
  if (base & 3) {
    const int64_t blocks = (n + kThreads - 1) / kThreads;  // <= 2^26
    hipLaunchKernelGGL(dropout_fwd_elem_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, st, x, y, n, keep, step,
                       seed, did, relu != 0, base);
    return (int)hipGetLastError();
  }
  const int vec = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0;
  const int64_t blocks = ((n + 3) / 4 + kThreads - 1) / kThreads;  // <= 2^24
  hipLaunchKernelGGL(dropout_fwd_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, st, x, y, n, keep, step, seed, did,
                     relu != 0, vec, base >> 2);
  return (int)hipGetLastError();
}

extern "C" int lbt_dropout_fwd(const float* x, float* y, int64_t n, float keep, const uint64_t* step, uint64_t seed,
                               uint32_t did, int32_t relu, void* stream) {
  return lbt_dropout_fwd_at(x, y, n, 0, keep, step, seed, did, relu, stream);
}

extern "C" int lbt_dropout_bwd_at(const float* g, float* dx, int64_t n, int64_t base, float keep, const uint64_t* step,
                                  uint64_t seed, uint32_t did, const float* relu_x, void* stream) {
  if (!window_ok(base, n) || !keep_ok(keep) || !step) return LBT_EINVAL;
  if (n == 0) return LBT_OK;
  hipStream_t st = (hipStream_t)stream;
  if (base & 3) {
    const int64_t blocks = (n + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(dropout_bwd_elem_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, st, g, dx, n, keep, step,
                       seed, did, relu_x, base);
    return (int)hipGetLastError();
  }
  const int vec = ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(dx) |
                    reinterpret_cast<uintptr_t>(relu_x)) & 15) == 0;
  const int64_t blocks = ((n + 3) / 4 + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(dropout_bwd_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, st, g, dx, n, keep, step, seed, did,
                     relu_x, vec, base >> 2);
  return (int)hipGetLastError();
}

extern "C" int lbt_dropout_bwd(const float* g, float* dx, int64_t n, float keep, const uint64_t* step, uint64_t seed,
                               uint32_t did, const float* relu_x, void* stream) {
  return lbt_dropout_bwd_at(g, dx, n, 0, keep, step, seed, did, relu_x, stream);
}

extern "C" int lbt_dropout_quantize_at(const float* x, void* out, int out_kind, int64_t rows, int64_t inner,
                                       int64_t base, float keep, uint32_t did, int32_t relu, lbt_qdesc q,
                                       void* stream) {
  if (rows < 0 || inner < 0 || base < 0 || base > kMaxN || !keep_ok(keep)) return LBT_EINVAL;
  if (out_kind != LBT_OUT_I8 && out_kind != LBT_OUT_U8OFF && out_kind != LBT_OUT_I16) return LBT_EINVAL;
  if (q.bits < 1 || q.bits > 16) return LBT_EINVAL;
  if ((out_kind == LBT_OUT_I8 && q.bits > 8) || (out_kind == LBT_OUT_U8OFF && q.bits > 9)) return LBT_EINVAL;
  if (rows == 0 || inner == 0) return LBT_OK;
  if (rows > (kMaxN - base) / inner) return LBT_EINVAL;  // base + n > 2^34
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = rows * inner;
  // the two paths, grids and rows per thread of lbt_dfxp_quantize: the same workgroup -> shard map
  const bool vec = (inner % 4 == 0) && (reinterpret_cast<uintptr_t>(x) % 16 == 0) && (inner >= 64) && !(base & 3);
  if (vec) {
    const int64_t groups = inner / 4;
    const int64_t gblocks = (groups + kThreads - 1) / kThreads;
    int64_t rpt = (gblocks * rows) / 512;
    if (rpt < 1) rpt = 1;
    if (rpt > 64) rpt = 64;
    const int64_t yblocks = (rows + rpt - 1) / rpt;
    if (yblocks > 65535) return LBT_EINVAL;
    hipLaunchKernelGGL(dropout_quantize_rows_kernel, dim3((unsigned)gblocks, (unsigned)yblocks), dim3(kThreads), 0, st,
                       x, out, out_kind, rows, inner, (int)rpt, keep, did, relu != 0, q, base);
  } else {
    int64_t blocks = (n + kThreads - 1) / kThreads;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(dropout_quantize_generic_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, st, x, out,
                       out_kind, n, inner, keep, did, relu != 0, q, base);
  }
  return (int)hipGetLastError();
}

extern "C" int lbt_dropout_quantize(const float* x, void* out, int out_kind, int64_t rows, int64_t inner, float keep,
                                    uint32_t did, int32_t relu, lbt_qdesc q, void* stream) {
  return lbt_dropout_quantize_at(x, out, out_kind, rows, inner, 0, keep, did, relu, q, stream);
}
