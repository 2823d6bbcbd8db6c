// batch_input.hip -- the input side of the epoch loop, from a dataset that lives on the device:
//
//   lbt_batch_gather   load_data's normalisation (main.py:65-75), the batch gather of the epoch loop
//                      (trainer.py:98-99) and preprocess_image (trainer.py:24-28) in one pass: the
//                      batch the step reads is written once, from the dataset's native uint8
//   lbt_batch_resized_crop   the ImageNet pipeline (data.py:58-93) the same way: RandomResizedCrop +
//                      RandomHorizontalFlip (training) or a centre crop (validation), a bilinear resample
//                      to the output size and Normalize(mean, std), all in integers up to one float64
//                      subtract-multiply per element (below, at its kernel)
//
// lbt_batch_gather: one workgroup per output sample: the source index and the Philox draw depend on blockIdx only, so
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

// ------------------------------------------------------------------ lbt_batch_resized_crop
// Everything up to the normalisation is integer arithmetic on values the host prepared (lbt_dfxp.h), so
// the numpy restatement (tests/resized_crop_oracle.py) agrees bit for bit whatever the compiler does.
//
// Grid (samples, row strips): a rank's shard of 32 samples is 32 workgroups on 256 CUs, so the host cuts
// every sample into strips of `rows` output rows until about 1024 workgroups exist. The box and the flip
// depend on blockIdx.x and the arguments only: wave-uniform, recomputed by every strip of a sample (two
// Philox calls, two integer roots and one 64-bit division per accepted attempt). Each workgroup then
// resolves the bilinear taps once into LDS -- one packed word (x0 | fx << 13 | (x1 - x0) << 22) per output
// column, the flip folded in, and one per row of its strip. A thread then owns one store position of the
// row and walks down the strip (see the loop), so the per-element work is four byte loads, six integer
// multiply-adds and the float64 subtract-multiply. The box is at most Hs*Ws*C bytes and is read by every
// strip of its sample: it stays in cache. Stores as in batch_gather_kernel: 16 bytes per lane when rows
// are whole quads and X is aligned, else 4.
namespace {

constexpr int kRrcMaxRows = 4096;  // rows of a strip: Wo + rows words of LDS, <= 48 KB

struct RrcArgs {
  const uint8_t* data;
  const int32_t* labels;
  int64_t n_data;
  const int32_t* idx;
  int64_t first;
  float* X;
  int32_t* y;
  uint32_t Hs, Ws, C, Ho, Wo, rows;
  int augment;
  uint32_t a_lo, a_span;  // area = a_lo + r.x % a_span
  const uint32_t* ratio;  // [256] aspect ratios, Q16
  uint32_t q_lo, q_hi;
  uint32_t ch, cw;
  const double* shift;
  const double* scale;
  int64_t base;
  uint64_t seed, counter;
};

struct Box { uint32_t top, left, h, w; };

// floor(sqrt(x)), x < 2^62: the float64 root is within one of it, the loops settle the rest exactly
LBT_DEV uint64_t isqrt64(uint64_t x) {
  uint64_t s = (uint64_t)sqrt((double)x);
  while (s * s > x) --s;
  while ((s + 1) * (s + 1) <= x) ++s;
  return s;
}

// The crop box of sample n: RandomResizedCrop.get_params in integers, or the central (ch, cw) box.
LBT_DEV Box rrc_box(const RrcArgs& a, uint32_t n) {
  const uint64_t Hs = a.Hs, Ws = a.Ws;
  if (!a.augment) return Box{(a.Hs - a.ch) / 2, (a.Ws - a.cw) / 2, a.ch, a.cw};
  for (uint32_t t = 0; t < 10; ++t) {
    const U4 r = philox(n, kRrcStream + t, (uint32_t)a.counter, (uint32_t)(a.counter >> 32), (uint32_t)a.seed,
                        (uint32_t)(a.seed >> 32));
    const uint64_t area = (uint64_t)a.a_lo + r.x % a.a_span;  // <= Hs*Ws <= 2^26
    const uint64_t q = a.ratio[r.y >> 24];
    if (q == 0) continue;  // (no table the host builds holds one: q >= q_lo >= 1)
    const uint64_t w = (isqrt64((4 * area * q) >> 16) + 1) >> 1;  // rint(sqrt(area * ratio)); 4aq < 2^60
    const uint64_t h = (isqrt64(((4 * area) << 16) / q) + 1) >> 1;  // rint(sqrt(area / ratio))
    if (w >= 1 && w <= Ws && h >= 1 && h <= Hs)
      return Box{(uint32_t)(r.z % (uint32_t)(Hs - h + 1)), (uint32_t)(r.w % (uint32_t)(Ws - w + 1)), (uint32_t)h,
                 (uint32_t)w};
  }
  uint64_t w = Ws, h = Hs;  // ten rejections: torchvision's central crop at the nearest allowed ratio
  if (Ws * 65536 < (uint64_t)a.q_lo * Hs) {
    h = (2 * Ws * 65536 + a.q_lo) / (2 * (uint64_t)a.q_lo);
    h = h > Hs ? Hs : h < 1 ? 1 : h;  // (< 1: ratios beyond 2 * Ws only; the box must hold a pixel)
  } else if (Ws * 65536 > (uint64_t)a.q_hi * Hs) {
    w = (2 * Hs * a.q_hi + 65536) >> 17;
    w = w > Ws ? Ws : w < 1 ? 1 : w;
  }
  return Box{(uint32_t)(Hs - h) / 2, (uint32_t)(Ws - w) / 2, (uint32_t)h, (uint32_t)w};
}

// Output index i of `out` samples across `in` source pixels, half-pixel centres: the lower tap, the weight
// of the upper one in 1/256 and whether the upper tap is another pixel. (2i + 1) * in <= 2^27.
LBT_DEV uint32_t rrc_tap(uint32_t i, uint32_t in, uint32_t out) {
  int32_t n = (int32_t)((2 * i + 1) * in) - (int32_t)out;
  const int32_t hi = (int32_t)((in - 1) * 2 * out);
  n = n < 0 ? 0 : n > hi ? hi : n;
  const uint32_t p0 = (uint32_t)n / (2 * out);
  const uint32_t f = (((uint32_t)n - p0 * 2 * out) * 256 + out) / (2 * out);
  return p0 | f << 13 | (p0 + 1 <= in - 1 ? 1u : 0u) << 22;
}

template <bool VEC>
__global__ __launch_bounds__(kT) void resized_crop_kernel(const RrcArgs a) {
  extern __shared__ uint32_t tab[];  // [Wo] column taps, [rows] this strip's row taps
  const uint32_t b = blockIdx.x, i0 = blockIdx.y * a.rows;
  const uint32_t nrow = a.Ho - i0 < a.rows ? a.Ho - i0 : a.rows;
  const int64_t s = a.idx ? (int64_t)a.idx[b] : a.first + (int64_t)b;
  const bool ok = s >= 0 && s < a.n_data;
  const uint32_t key = (uint32_t)(a.base + (int64_t)b);
  const Box box = rrc_box(a, key);
  const bool fl = a.augment && (philox(key, kAugStream, (uint32_t)a.counter, (uint32_t)(a.counter >> 32),
                                       (uint32_t)a.seed, (uint32_t)(a.seed >> 32)).x & 1u);
  for (uint32_t j = threadIdx.x; j < a.Wo; j += kT) tab[j] = rrc_tap(fl ? a.Wo - 1 - j : j, box.w, a.Wo);
  for (uint32_t i = threadIdx.x; i < nrow; i += kT) tab[a.Wo + i] = rrc_tap(i0 + i, box.h, a.Ho);
  if (blockIdx.y == 0 && threadIdx.x == 0) a.y[b] = ok ? a.labels[s] : -1;
  __syncthreads();
  const uint32_t WoC = a.Wo * a.C, rs = a.Ws * a.C, total = nrow * WoC;  // < 2^31 (host checks)
  const uint8_t* __restrict__ src =
      a.data + (ok ? s * (int64_t)a.Hs * rs : 0) + ((int64_t)box.top * a.Ws + box.left) * a.C;
  float* __restrict__ out = a.X + ((int64_t)b * a.Ho + i0) * (int64_t)WoC;
  constexpr uint32_t kV = VEC ? 4u : 1u;
  if (!ok) {  // (uniform) nothing to read: a zero image
    for (uint32_t e = threadIdx.x * kV; e < total; e += kT * kV) {
      if constexpr (VEC) {
        *reinterpret_cast<float4*>(out + e) = make_float4(0.f, 0.f, 0.f, 0.f);
      } else {
        out[e] = 0.f;
      }
    }
    return;
  }
  // A thread keeps one store position of the row -- its elements' column taps, channel constants and
  // source offsets in registers -- and walks down the strip's rows: per row one LDS read and, per element,
  // four byte loads (32-bit offsets from the uniform box origin, all in flight together) and the
  // arithmetic; nothing is divided and no column tap is read again. The workgroup is a (rows in flight) x
  // (stores per row) grid of threads; a row of more than kT stores takes several passes.
  const uint32_t Q = WoC / kV, Qc = Q < (uint32_t)kT ? Q : (uint32_t)kT, G = (uint32_t)kT / Qc;
  const uint32_t g = threadIdx.x / Qc, q0 = threadIdx.x - g * Qc;
  if (g >= G) return;
  for (uint32_t q = q0; q < Q; q += Qc) {
    const uint32_t e0 = q * kV;
    uint32_t j = e0 / a.C, c = e0 - j * a.C;
    uint32_t x0[kV], x1[kV];
    int32_t fx[kV];
    double sh[kV], sc[kV];
#pragma unroll
    for (uint32_t k = 0; k < kV; ++k) {  // VEC: WoC % 4 == 0, the quad stays inside its row
      const uint32_t tx = tab[j];
      x0[k] = (tx & 8191u) * a.C + c;
      x1[k] = x0[k] + (tx >> 22) * a.C;
      fx[k] = (int32_t)((tx >> 13) & 511u);
      sh[k] = a.shift[c];
      sc[k] = a.scale[c];
      if (++c == a.C) { c = 0; ++j; }
    }
    for (uint32_t il = g; il < nrow; il += G) {
      const uint32_t ty = tab[a.Wo + il];
      const uint32_t row0 = (ty & 8191u) * rs, row1 = row0 + (ty >> 22) * rs;
      const int32_t fy = (int32_t)((ty >> 13) & 511u);
      int32_t p00[kV], p01[kV], p10[kV], p11[kV];
#pragma unroll
      for (uint32_t k = 0; k < kV; ++k) {
        p00[k] = src[row0 + x0[k]];
        p01[k] = src[row0 + x1[k]];
        p10[k] = src[row1 + x0[k]];
        p11[k] = src[row1 + x1[k]];
      }
      float v[kV];
#pragma unroll
      for (uint32_t k = 0; k < kV; ++k) {
        const int32_t top = (256 - fx[k]) * p00[k] + fx[k] * p01[k];
        const int32_t bot = (256 - fx[k]) * p10[k] + fx[k] * p11[k];
        const int32_t acc = (int32_t)(__umul24(256 - fy, top) + __umul24(fy, bot));  // factors < 2^24; <= 255 * 65536
        v[k] = (float)(((double)acc - sh[k]) * sc[k]);
      }
      float* __restrict__ o = out + il * WoC + e0;
      if constexpr (VEC) {
        *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
      } else {
        *o = v[0];
      }
    }
  }
}

}  // namespace

extern "C" int lbt_batch_resized_crop(const uint8_t* data, const int32_t* labels, int64_t n_data, const int32_t* idx,
                                      int64_t first, float* X, int32_t* y, int32_t B, int32_t Hs, int32_t Ws, int32_t C,
                                      int32_t Ho, int32_t Wo, int32_t augment, int64_t a_lo, int64_t a_hi,
                                      const uint32_t* ratio_q16, int64_t q_lo, int64_t q_hi, int32_t ch, int32_t cw,
                                      const double* shift, const double* scale_c, int64_t base, uint64_t seed,
                                      uint64_t counter, void* stream) {
  if (!data || !labels || !X || !y || !ratio_q16 || !shift || !scale_c) return LBT_EINVAL;
  if (B <= 0 || Hs <= 0 || Ws <= 0 || C <= 0 || Ho <= 0 || Wo <= 0 || n_data <= 0) return LBT_EINVAL;
  if (Hs > 8192 || Ws > 8192 || Ho > 8192 || Wo > 8192) return LBT_EINVAL;
  if ((int64_t)Hs * Ws * C >= ((int64_t)1 << 31) || (int64_t)Ho * Wo * C >= ((int64_t)1 << 31)) return LBT_EINVAL;
  if (a_lo < 1 || a_hi < a_lo || a_hi > (int64_t)Hs * Ws) return LBT_EINVAL;
  if (q_lo < 1 || q_hi < q_lo || q_hi > 0xFFFFFFFFLL) return LBT_EINVAL;
  if (ch < 1 || ch > Hs || cw < 1 || cw > Ws) return LBT_EINVAL;
  if (base < 0 || base > ((int64_t)1 << 32) - B) return LBT_EINVAL;  // the draw's key is 32 bits wide
  if (!idx && (first < 0 || first > n_data - B)) return LBT_EINVAL;
  // strips: about 1024 workgroups (four per CU) however small the batch; 2048 measured slower: every strip redoes the box
  const int32_t want = (1024 + B - 1) / B;
  int32_t rows = (Ho + want - 1) / want;
  rows = rows < 1 ? 1 : rows > kRrcMaxRows ? kRrcMaxRows : rows;
  const int32_t strips = (Ho + rows - 1) / rows;
  RrcArgs a;
  a.data = data; a.labels = labels; a.n_data = n_data; a.idx = idx; a.first = first; a.X = X; a.y = y;
  a.Hs = (uint32_t)Hs; a.Ws = (uint32_t)Ws; a.C = (uint32_t)C; a.Ho = (uint32_t)Ho; a.Wo = (uint32_t)Wo;
  a.rows = (uint32_t)rows; a.augment = augment != 0;
  a.a_lo = (uint32_t)a_lo; a.a_span = (uint32_t)(a_hi - a_lo + 1);
  a.ratio = ratio_q16; a.q_lo = (uint32_t)q_lo; a.q_hi = (uint32_t)q_hi; a.ch = (uint32_t)ch; a.cw = (uint32_t)cw;
  a.shift = shift; a.scale = scale_c; a.base = base; a.seed = seed; a.counter = counter;
  const bool vec = ((int64_t)Wo * C) % 4 == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0;
  const dim3 grid((unsigned)B, (unsigned)strips);
  const size_t lds = sizeof(uint32_t) * (size_t)(Wo + rows);
  if (vec)
    hipLaunchKernelGGL((resized_crop_kernel<true>), grid, dim3(kT), lds, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL((resized_crop_kernel<false>), grid, dim3(kT), lds, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}
