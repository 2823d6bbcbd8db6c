// batch_input.hip -- the input side of the epoch loop, from a dataset that lives on the device:
//
//   lbt_batch_gather   load_data's normalisation (main.py:65-75), the batch gather of the epoch loop
//                      (trainer.py:98-99) and preprocess_image (trainer.py:24-28) in one pass: the
//                      batch the step reads is written once, from the dataset's native uint8
//
// One workgroup per output sample: the source index and the Philox draw depend on blockIdx only, so
// they are wave-uniform. A streaming pass bound by its stores (4 B written per byte read): each lane
// writes four consecutive floats of the flattened image with one 16-byte store when rows are whole
// quads and X is 16-byte aligned, else one float. Source elements are gathered one by one (a flip
// reverses pixels, not channels); an image is a few KB and stays in cache. No LDS.
#include "dfxp_device.h"

using namespace lbt;

namespace {

constexpr int kT = 256;

// Normalised value of element p of the source image at data + img (elements).
// KIND 0: load_data's float64 (u8 - mean) / 128, rounded to fp32 once (1 / 128 is a power of two: the
// product is the quotient). KIND 1: the stored float.
template <int KIND>
LBT_DEV float load_norm(const void* __restrict__ data, const double* __restrict__ mean, int64_t img, uint32_t p) {
  if (KIND == 0) {
    const double u = (double)static_cast<const uint8_t*>(data)[img + p];
    return (float)((u - mean[p]) * (1.0 / 128));
  }
  return static_cast<const float*>(data)[img + p];
}

// y[b] = labels[s], X[b] = crop(pad(flip(norm(data[s])))) with s = idx ? idx[b] : first + b and the
// draw of sample base + b (augment_kernel's, aux.hip). An s outside [0, n_data) -- the host cannot
// see idx's values -- reads nothing: the image is zero and the label -1.
template <int KIND, bool VEC>
__global__ __launch_bounds__(kT) void batch_gather_kernel(const void* __restrict__ data,
                                                          const double* __restrict__ mean,
                                                          const int32_t* __restrict__ labels, int64_t n_data,
                                                          const int32_t* __restrict__ idx, int64_t first,
                                                          float* __restrict__ X, int32_t* __restrict__ y, int H, int W,
                                                          int C, int pad, int flip, int64_t base, uint64_t seed,
                                                          uint64_t counter) {
  const uint32_t b = blockIdx.x;
  const int64_t s = idx ? (int64_t)idx[b] : first + (int64_t)b;
  const bool ok = s >= 0 && s < n_data;
  const U4 r = philox((uint32_t)(base + (int64_t)b), kAugStream, (uint32_t)counter, (uint32_t)(counter >> 32),
                      (uint32_t)seed, (uint32_t)(seed >> 32));
  const uint32_t span = 2u * (uint32_t)pad + 1u;
  const bool fl = flip && (r.x & 1u);
  const int dy = (int)(r.y % span) - pad, dx = (int)(r.z % span) - pad;
  const uint32_t WC = (uint32_t)W * (uint32_t)C, HWC = (uint32_t)H * WC;  // < 2^31 (host check)
  const int64_t img = ok ? s * (int64_t)HWC : 0;
  float* __restrict__ out = X + (int64_t)b * (int64_t)HWC;
  if (threadIdx.x == 0) y[b] = ok ? labels[s] : -1;
  constexpr uint32_t kV = VEC ? 4u : 1u;
  for (uint32_t e = threadIdx.x * kV; e < HWC; e += kT * kV) {  // e + kT * kV < 2^32
    const uint32_t i = e / WC, r0 = e - i * WC;
    uint32_t j = r0 / (uint32_t)C, c = r0 - j * (uint32_t)C;
    const int si = (int)i + dy;
    const bool row_ok = ok && si >= 0 && si < H;
    float v[kV];
#pragma unroll
    for (uint32_t k = 0; k < kV; ++k) {  // VEC: WC % 4 == 0, the quad stays inside row i
      const int sj0 = (int)j + dx;
      float t = 0.f;
      if (row_ok && sj0 >= 0 && sj0 < W) {
        const uint32_t sj = (uint32_t)(fl ? W - 1 - sj0 : sj0);
        t = load_norm<KIND>(data, mean, img, ((uint32_t)si * (uint32_t)W + sj) * (uint32_t)C + c);
      }
      v[k] = t;
      if (++c == (uint32_t)C) { c = 0; ++j; }
    }
    if constexpr (VEC) {
      *reinterpret_cast<float4*>(out + e) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      out[e] = v[0];
    }
  }
}

template <int KIND>
int launch(bool vec, int32_t B, hipStream_t st, const void* data, const double* mean, const int32_t* labels,
           int64_t n_data, const int32_t* idx, int64_t first, float* X, int32_t* y, int H, int W, int C, int pad, int flip,
           int64_t base, uint64_t seed, uint64_t counter) {
  if (vec)
    hipLaunchKernelGGL((batch_gather_kernel<KIND, true>), dim3((unsigned)B), dim3(kT), 0, st, data, mean, labels, n_data,
                       idx, first, X, y, H, W, C, pad, flip, base, seed, counter);
  else
    hipLaunchKernelGGL((batch_gather_kernel<KIND, false>), dim3((unsigned)B), dim3(kT), 0, st, data, mean, labels, n_data,
                       idx, first, X, y, H, W, C, pad, flip, base, seed, counter);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" int lbt_batch_gather(const void* data, int32_t src_kind, const double* mean, const int32_t* labels,
                                int64_t n_data, const int32_t* idx, int64_t first, float* X, int32_t* y, int32_t B,
                                int32_t H, int32_t W, int32_t C, int32_t pad, int32_t flip, int64_t base, uint64_t seed,
                                uint64_t counter, void* stream) {
  if (!data || !labels || !X || !y) return LBT_EINVAL;
  if (src_kind != 0 && src_kind != 1) return LBT_EINVAL;
  if (src_kind == 0 && !mean) return LBT_EINVAL;
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || n_data <= 0) return LBT_EINVAL;
  if (pad < 0 || pad >= 32768) return LBT_EINVAL;
  if (base < 0 || base > ((int64_t)1 << 32) - B) return LBT_EINVAL;  // the draw's key is 32 bits wide
  if (!idx && (first < 0 || first > n_data - B)) return LBT_EINVAL;
  if ((int64_t)H * W >= ((int64_t)1 << 31) || (int64_t)H * W * C >= ((int64_t)1 << 31)) return LBT_EINVAL;
  const bool vec = ((int64_t)W * C) % 4 == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0;
  hipStream_t st = (hipStream_t)stream;
  return src_kind == 0 ? launch<0>(vec, B, st, data, mean, labels, n_data, idx, first, X, y, H, W, C, pad, flip, base,
                                   seed, counter)
                       : launch<1>(vec, B, st, data, mean, labels, n_data, idx, first, X, y, H, W, C, pad, flip, base,
                                   seed, counter);
}
