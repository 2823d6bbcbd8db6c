// batch_input.hip -- the input side of the epoch loop, from a dataset that lives on the device:
//
//   lbt_batch_gather   load_data's normalisation (main.py:65-75), the batch gather of the epoch loop
//                      (trainer.py:98-99) and preprocess_image (trainer.py:24-28) in one pass: the
//                      batch the step reads is written once, from the dataset's native uint8
//   lbt_batch_resized_crop   the ImageNet pipeline (data.py:58-93) the same way: RandomResizedCrop +
//                      RandomHorizontalFlip (training) or a centre crop (validation), a bilinear resample
//                      to the output size and Normalize(mean, std), all in integers up to one float64
//                      subtract-multiply per element (below, at its kernel)
//   lbt_batch_resized_crop_jitter   the same with ColorJitter's brightness, contrast and saturation between the
//                      resample and the normalisation, in integers (at the end of this file)
//   lbt_batch_ragged_crop (+ _jitter)   the same two on a store of images of differing size: the same kernels,
//                      instantiated to read each sample's geometry from a table (rrc_geom)
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

// A ragged store's launch: [n_data] records in place of Hs, Ws, a_lo, a_span, ch, cw (which it leaves unread).
// Appended, so that the uniform kernels keep the argument block, and with it the code, they had.
struct RaggedArgs : RrcArgs {
  const lbt_image_geom* geom;
  int64_t data_bytes;
};

template <bool RAGGED>
using RrcArgsT = std::conditional_t<RAGGED, RaggedArgs, RrcArgs>;

struct Box { uint32_t top, left, h, w; };

// What a ragged store has per image and a uniform one per launch. A function of the source sample, which is a
// function of blockIdx.x and the arguments: wave-uniform, like everything derived from it (the box, the row
// stride, the 64-bit image base). A RAGGED kernel reads it from the table with scalar loads -- the address
// holds no lane index and nothing the kernel stores precedes the load -- and the uniform instantiation
// copies its arguments (and forms the image base where it always did: img stays unused).
struct Geom {
  uint32_t Hs, Ws, a_lo, a_span, ch, cw;
  const uint8_t* img;  // RAGGED: the image's first pixel
  bool ok;             // there is an image to read
};

template <bool RAGGED>
LBT_DEV Geom rrc_geom(const RrcArgsT<RAGGED>& a, int64_t s) {
  const bool ok = s >= 0 && s < a.n_data;
  if constexpr (!RAGGED) {
    return Geom{a.Hs, a.Ws, a.a_lo, a.a_span, a.ch, a.cw, nullptr, ok};
  } else {
    const Geom none{1, 1, 1, 1, 1, 1, a.data, false};  // a box of one pixel that is never read
    if (!ok) return none;
    const lbt_image_geom r = a.geom[s];
    // The host cannot see the table (lbt_dfxp.h): a record lbt_image_geom_check would refuse is not read through.
    const int64_t px = (int64_t)r.Hs * r.Ws;
    if (r.Hs < 1 || r.Hs > 8192 || r.Ws < 1 || r.Ws > 8192 || r.offset < 0 || px * a.C >= ((int64_t)1 << 31) ||
        r.offset > a.data_bytes - px * a.C || r.a_lo < 1 || r.a_hi < r.a_lo || r.a_hi > px || r.ch < 1 || r.ch > r.Hs ||
        r.cw < 1 || r.cw > r.Ws)
      return none;
    return Geom{(uint32_t)r.Hs, (uint32_t)r.Ws, (uint32_t)r.a_lo, (uint32_t)(r.a_hi - r.a_lo + 1), (uint32_t)r.ch,
                (uint32_t)r.cw, a.data + r.offset, true};
  }
}

// floor(sqrt(x)), x < 2^62: the float64 root is within one of it, the loops settle the rest exactly
LBT_DEV uint64_t isqrt64(uint64_t x) {
  uint64_t s = (uint64_t)sqrt((double)x);
  while (s * s > x) --s;
  while ((s + 1) * (s + 1) <= x) ++s;
  return s;
}

// The crop box of sample n: RandomResizedCrop.get_params in integers, or the central (ch, cw) box.
LBT_DEV Box rrc_box(const RrcArgs& a, const Geom& g, uint32_t n) {
  const uint64_t Hs = g.Hs, Ws = g.Ws;
  if (!a.augment) return Box{(g.Hs - g.ch) / 2, (g.Ws - g.cw) / 2, g.ch, g.cw};
  for (uint32_t t = 0; t < 10; ++t) {
    const U4 r = philox(n, kRrcStream + t, (uint32_t)a.counter, (uint32_t)(a.counter >> 32), (uint32_t)a.seed,
                        (uint32_t)(a.seed >> 32));
    const uint64_t area = (uint64_t)g.a_lo + r.x % g.a_span;  // <= Hs*Ws <= 2^26
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

template <bool VEC, bool RAGGED>
__global__ __launch_bounds__(kT) void resized_crop_kernel(const RrcArgsT<RAGGED> a) {
  extern __shared__ uint32_t tab[];  // [Wo] column taps, [rows] this strip's row taps
  const uint32_t b = blockIdx.x, i0 = blockIdx.y * a.rows;
  const uint32_t nrow = a.Ho - i0 < a.rows ? a.Ho - i0 : a.rows;
  const int64_t s = a.idx ? (int64_t)a.idx[b] : a.first + (int64_t)b;
  const Geom gm = rrc_geom<RAGGED>(a, s);
  const bool ok = gm.ok;
  const uint32_t key = (uint32_t)(a.base + (int64_t)b);
  const Box box = rrc_box(a, gm, key);
  const bool fl = a.augment && (philox(key, kAugStream, (uint32_t)a.counter, (uint32_t)(a.counter >> 32),
                                       (uint32_t)a.seed, (uint32_t)(a.seed >> 32)).x & 1u);
  for (uint32_t j = threadIdx.x; j < a.Wo; j += kT) tab[j] = rrc_tap(fl ? a.Wo - 1 - j : j, box.w, a.Wo);
  for (uint32_t i = threadIdx.x; i < nrow; i += kT) tab[a.Wo + i] = rrc_tap(i0 + i, box.h, a.Ho);
  if (blockIdx.y == 0 && threadIdx.x == 0) a.y[b] = ok ? a.labels[s] : -1;
  __syncthreads();
  const uint32_t WoC = a.Wo * a.C, rs = gm.Ws * a.C, total = nrow * WoC;  // < 2^31 (host checks)
  const uint8_t* img = gm.img;
  if constexpr (!RAGGED) img = a.data + (ok ? s * (int64_t)a.Hs * rs : 0);  // (formed here, as it always was)
  const uint8_t* __restrict__ src = img + ((int64_t)box.top * gm.Ws + box.left) * a.C;
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

// rows of a strip: about 1024 workgroups (four per CU) however small the batch; 2048 measured slower: every
// strip redoes the box. A function of B and Ho alone, which the jitter's scratch size follows.
int32_t rrc_strip_rows(int32_t B, int32_t Ho) {
  const int32_t want = (1024 + B - 1) / B;
  const int32_t rows = (Ho + want - 1) / want;
  return rows < 1 ? 1 : rows > kRrcMaxRows ? kRrcMaxRows : rows;
}

// What the entry points share, checked and packed: everything but the store's geometry. false: LBT_EINVAL.
bool rrc_pack(RrcArgs& a, const uint8_t* data, const int32_t* labels, int64_t n_data, const int32_t* idx, int64_t first,
              float* X, int32_t* y, int32_t B, int32_t C, int32_t Ho, int32_t Wo, int32_t augment,
              const uint32_t* ratio_q16, int64_t q_lo, int64_t q_hi, const double* shift, const double* scale_c,
              int64_t base, uint64_t seed, uint64_t counter) {
  if (!data || !labels || !X || !y || !ratio_q16 || !shift || !scale_c) return false;
  if (B <= 0 || C <= 0 || Ho <= 0 || Wo <= 0 || n_data <= 0) return false;
  if (Ho > 8192 || Wo > 8192 || (int64_t)Ho * Wo * C >= ((int64_t)1 << 31)) return false;
  if (q_lo < 1 || q_hi < q_lo || q_hi > 0xFFFFFFFFLL) return false;
  if (base < 0 || base > ((int64_t)1 << 32) - B) return false;  // the draw's key is 32 bits wide
  if (!idx && (first < 0 || first > n_data - B)) return false;
  a.data = data; a.labels = labels; a.n_data = n_data; a.idx = idx; a.first = first; a.X = X; a.y = y;
  a.C = (uint32_t)C; a.Ho = (uint32_t)Ho; a.Wo = (uint32_t)Wo;
  a.rows = (uint32_t)rrc_strip_rows(B, Ho); a.augment = augment != 0;
  a.ratio = ratio_q16; a.q_lo = (uint32_t)q_lo; a.q_hi = (uint32_t)q_hi;
  a.shift = shift; a.scale = scale_c; a.base = base; a.seed = seed; a.counter = counter;
  a.Hs = a.Ws = a.a_lo = a.a_span = a.ch = a.cw = 0;
  return true;
}

// One stored size for every image (C as rrc_pack checked it)
bool rrc_pack_uniform(RrcArgs& a, int32_t Hs, int32_t Ws, int64_t a_lo, int64_t a_hi, int32_t ch, int32_t cw) {
  if (Hs <= 0 || Ws <= 0 || Hs > 8192 || Ws > 8192 || (int64_t)Hs * Ws * a.C >= ((int64_t)1 << 31)) return false;
  if (a_lo < 1 || a_hi < a_lo || a_hi > (int64_t)Hs * Ws) return false;
  if (ch < 1 || ch > Hs || cw < 1 || cw > Ws) return false;
  a.Hs = (uint32_t)Hs; a.Ws = (uint32_t)Ws; a.a_lo = (uint32_t)a_lo; a.a_span = (uint32_t)(a_hi - a_lo + 1);
  a.ch = (uint32_t)ch; a.cw = (uint32_t)cw;
  return true;
}

// A table of sizes: its records are on the device, so only the pointer and the size can be refused here
bool rrc_pack_ragged(RaggedArgs& a, const lbt_image_geom* geom, int64_t data_bytes) {
  if (!geom || data_bytes <= 0) return false;
  a.geom = geom; a.data_bytes = data_bytes;
  return true;
}

dim3 rrc_grid(const RrcArgs& a, int32_t B) { return dim3((unsigned)B, (unsigned)((a.Ho + a.rows - 1) / a.rows)); }
size_t rrc_lds(const RrcArgs& a) { return sizeof(uint32_t) * (size_t)(a.Wo + a.rows); }

template <bool RAGGED>
int rrc_launch(const RrcArgsT<RAGGED>& a, int32_t B, void* stream) {
  const bool vec = ((int64_t)a.Wo * a.C) % 4 == 0 && (reinterpret_cast<uintptr_t>(a.X) & 15) == 0;
  if (vec)
    hipLaunchKernelGGL((resized_crop_kernel<true, RAGGED>), rrc_grid(a, B), dim3(kT), rrc_lds(a), (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL((resized_crop_kernel<false, RAGGED>), rrc_grid(a, B), dim3(kT), rrc_lds(a), (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" int lbt_batch_resized_crop(const uint8_t* data, const int32_t* labels, int64_t n_data, const int32_t* idx,
                                      int64_t first, float* X, int32_t* y, int32_t B, int32_t Hs, int32_t Ws, int32_t C,
                                      int32_t Ho, int32_t Wo, int32_t augment, int64_t a_lo, int64_t a_hi,
                                      const uint32_t* ratio_q16, int64_t q_lo, int64_t q_hi, int32_t ch, int32_t cw,
                                      const double* shift, const double* scale_c, int64_t base, uint64_t seed,
                                      uint64_t counter, void* stream) {
  RrcArgs a;
  if (!rrc_pack(a, data, labels, n_data, idx, first, X, y, B, C, Ho, Wo, augment, ratio_q16, q_lo, q_hi, shift, scale_c,
                base, seed, counter) ||
      !rrc_pack_uniform(a, Hs, Ws, a_lo, a_hi, ch, cw))
    return LBT_EINVAL;
  return rrc_launch<false>(a, B, stream);
}

extern "C" int lbt_batch_ragged_crop(const uint8_t* data, int64_t data_bytes, const lbt_image_geom* geom,
                                     const int32_t* labels, int64_t n_data, const int32_t* idx, int64_t first, float* X,
                                     int32_t* y, int32_t B, int32_t C, int32_t Ho, int32_t Wo, int32_t augment,
                                     const uint32_t* ratio_q16, int64_t q_lo, int64_t q_hi, const double* shift,
                                     const double* scale_c, int64_t base, uint64_t seed, uint64_t counter,
                                     void* stream) {
  RaggedArgs a;
  if (!rrc_pack(a, data, labels, n_data, idx, first, X, y, B, C, Ho, Wo, augment, ratio_q16, q_lo, q_hi, shift, scale_c,
                base, seed, counter) ||
      !rrc_pack_ragged(a, geom, data_bytes))
    return LBT_EINVAL;
  return rrc_launch<true>(a, B, stream);
}

extern "C" int64_t lbt_image_geom_check(const lbt_image_geom* host_geom, int64_t n_data, int32_t C, int64_t data_bytes) {
  if (!host_geom || n_data <= 0 || C <= 0 || data_bytes <= 0) return -2;
  for (int64_t i = 0; i < n_data; ++i) {
    const lbt_image_geom& r = host_geom[i];
    if (r.Hs < 1 || r.Hs > 8192 || r.Ws < 1 || r.Ws > 8192) return i;
    const int64_t px = (int64_t)r.Hs * r.Ws, bytes = px * C;  // <= 2^26 * C: no overflow
    if (bytes >= ((int64_t)1 << 31) || r.offset < 0 || r.offset > data_bytes - bytes) return i;
    if (r.a_lo < 1 || r.a_hi < r.a_lo || r.a_hi > px) return i;
    if (r.ch < 1 || r.ch > r.Hs || r.cw < 1 || r.cw > r.Ws) return i;
  }
  return -1;
}

// ------------------------------------------------------------------ lbt_batch_resized_crop_jitter
// ColorJitter (brightness, contrast, saturation; lbt_dfxp.h) between the blend and the normalisation, on the
// grid, prologue and LDS tables of resized_crop_kernel (restated here: that kernel stays as it is). Saturation
// and grey need a pixel's three channels, so a thread owns whole pixels: four (48 contiguous, 16-byte aligned
// bytes per lane) when Wo is a multiple of four and X is aligned, else one (12 bytes, 4-byte aligned). The order and the factors are one
// Philox call per workgroup: wave-uniform, every branch on them is a scalar branch. Contrast needs the mean
// grey of the whole image, which is many workgroups: jitter_stats_kernel resamples its strip, applies what
// precedes contrast in the sample's order (jit_pixel_pre, the same function the output kernel calls) and
// writes the strip's integer sum of grey; jitter_out_kernel adds a sample's sums in a uniform loop. Integer
// sums: no order matters and nothing is zeroed. The stats pass repeats the loads and the blend of the output
// pass (the box is in cache) and stores nothing.
namespace {

constexpr int32_t kJitT = 255 * 65536;  // the largest blend value
constexpr int32_t kJitOne = 4096;       // Q12 factor 1: every operation returns t
constexpr uint32_t kJitStream = 0x434A5421u;  // "CJT!"
enum : uint32_t { kOpB = 0, kOpC = 1, kOpS = 2 };

template <bool RAGGED>
struct JitArgsT {
  RrcArgsT<RAGGED> r;
  uint32_t fb_lo, fb_span, fc_lo, fc_span, fs_lo, fs_span;  // factor = lo + draw % span
  uint64_t* work;  // [B][strips] sums of grey, or NULL with contrast off
  uint32_t strips;
};

// A sample's draw. seq: the order's three operations, two bits each, the first in the low bits; f: the three
// factors (<= 65536), 17 bits each, at 17 * operation -- shifts of a scalar, where three fields picked by the
// operation became an indexed read of a stack copy.
struct Jit {
  uint32_t seq, cpos;  // cpos: contrast's place in the order
  uint64_t f;
};

LBT_DEV int32_t jit_factor(const Jit& j, uint32_t op) { return (int32_t)((j.f >> (17 * op)) & 0x1FFFFu); }

template <class JitArgs>
LBT_DEV Jit jit_draw(const JitArgs& a, uint32_t key) {
  const U4 r = philox(key, kJitStream, (uint32_t)a.r.counter, (uint32_t)(a.r.counter >> 32), (uint32_t)a.r.seed,
                      (uint32_t)(a.r.seed >> 32));
  // BCS, BSC, CBS, CSB, SBC, SCB as (first | second << 2 | third << 4), six bits per order
  constexpr uint64_t kSeq = (uint64_t)(kOpB | kOpC << 2 | kOpS << 4) | (uint64_t)(kOpB | kOpS << 2 | kOpC << 4) << 6 |
                            (uint64_t)(kOpC | kOpB << 2 | kOpS << 4) << 12 | (uint64_t)(kOpC | kOpS << 2 | kOpB << 4) << 18 |
                            (uint64_t)(kOpS | kOpB << 2 | kOpC << 4) << 24 | (uint64_t)(kOpS | kOpC << 2 | kOpB << 4) << 30;
  Jit j;
  j.seq = (uint32_t)(kSeq >> (6 * (r.x % 6u))) & 63u;
  j.cpos = (j.seq & 3u) == kOpC ? 0u : ((j.seq >> 2) & 3u) == kOpC ? 1u : 2u;
  j.f = (uint64_t)(a.fb_lo + r.y % a.fb_span) << (17 * kOpB) | (uint64_t)(a.fc_lo + r.z % a.fc_span) << (17 * kOpC) |
        (uint64_t)(a.fs_lo + r.w % a.fs_span) << (17 * kOpS);
  return j;
}

// PIL's "L" weights (they sum to 65536: grey <= kJitT); 64-bit: 38470 * 2^24 > 2^32
LBT_DEV int32_t jit_grey(const int32_t (&t)[3]) {
  return (int32_t)((19595ull * (uint32_t)t[0] + 38470ull * (uint32_t)t[1] + 7471ull * (uint32_t)t[2] + 32768ull) >> 16);
}

// clamp(floor((4096 d + 2048 + f (t - d)) / 4096), 0, T): f < 2^17, |t - d| < 2^25, the shift of the signed
// sum is the floor
LBT_DEV int32_t jit_blend(int32_t t, int32_t d, int32_t f) {
  const int64_t v = (((int64_t)d << 12) + 2048 + (int64_t)f * (int64_t)(t - d)) >> 12;
  return v < 0 ? 0 : v > kJitT ? kJitT : (int32_t)v;
}

// Operation k of the sample's order on one pixel (uniform branches). A factor of one is skipped: it returns t.
LBT_DEV void jit_apply(const Jit& j, uint32_t k, int32_t M, int32_t (&t)[3]) {
  const uint32_t op = (j.seq >> (2 * k)) & 3u;
  const int32_t f = jit_factor(j, op);
  if (f == kJitOne) return;
  const int32_t d = op == kOpB ? 0 : op == kOpC ? M : jit_grey(t);
#pragma unroll
  for (int c = 0; c < 3; ++c) t[c] = jit_blend(t[c], d, f);
}

// One output pixel as it stands when contrast's turn comes: the bilinear blend of its three channels
// (resized_crop_kernel's arithmetic; x0 / x1 are the taps' byte offsets of channel 0), then the operations
// before contrast in the sample's order. Both kernels call this.
LBT_DEV void jit_pixel_pre(const uint8_t* __restrict__ src, uint32_t row0, uint32_t row1, int32_t fy, uint32_t x0,
                           uint32_t x1, int32_t fx, const Jit& j, int32_t (&t)[3]) {
  int32_t p00[3], p01[3], p10[3], p11[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    p00[c] = src[row0 + x0 + c];
    p01[c] = src[row0 + x1 + c];
    p10[c] = src[row1 + x0 + c];
    p11[c] = src[row1 + x1 + c];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int32_t top = (256 - fx) * p00[c] + fx * p01[c];
    const int32_t bot = (256 - fx) * p10[c] + fx * p11[c];
    t[c] = (int32_t)(__umul24(256 - fy, top) + __umul24(fy, bot));  // factors < 2^24; <= 255 * 65536
  }
#pragma unroll
  for (uint32_t k = 0; k < 2; ++k)
    if (k < j.cpos) jit_apply(j, k, 0, t);
}

// What every strip of a sample resolves first, as resized_crop_kernel does: source sample, box, flip and the
// tap tables in LDS; here also the jitter's draw. Ends in the barrier that publishes the tables.
struct JitStrip {
  uint32_t i0, nrow;
  bool ok;
  const uint8_t* src;
  uint32_t rs;  // the source image's row stride in bytes
  Jit j;
};

template <bool RAGGED>
LBT_DEV JitStrip jit_prologue(const JitArgsT<RAGGED>& ja, uint32_t* tab, bool write_label) {
  const RrcArgsT<RAGGED>& a = ja.r;
  JitStrip s;
  const uint32_t b = blockIdx.x;
  s.i0 = blockIdx.y * a.rows;
  s.nrow = a.Ho - s.i0 < a.rows ? a.Ho - s.i0 : a.rows;
  const int64_t sm = a.idx ? (int64_t)a.idx[b] : a.first + (int64_t)b;
  const Geom gm = rrc_geom<RAGGED>(a, sm);
  s.ok = gm.ok;
  const uint32_t key = (uint32_t)(a.base + (int64_t)b);
  const Box box = rrc_box(a, gm, key);
  const bool fl = a.augment && (philox(key, kAugStream, (uint32_t)a.counter, (uint32_t)(a.counter >> 32),
                                       (uint32_t)a.seed, (uint32_t)(a.seed >> 32)).x & 1u);
  s.j = jit_draw(ja, key);
  for (uint32_t j = threadIdx.x; j < a.Wo; j += kT) tab[j] = rrc_tap(fl ? a.Wo - 1 - j : j, box.w, a.Wo);
  for (uint32_t i = threadIdx.x; i < s.nrow; i += kT) tab[a.Wo + i] = rrc_tap(s.i0 + i, box.h, a.Ho);
  if (write_label && blockIdx.y == 0 && threadIdx.x == 0) a.y[b] = s.ok ? a.labels[sm] : -1;
  __syncthreads();
  const uint8_t* img = gm.img;
  if constexpr (!RAGGED) img = a.data + (s.ok ? sm * (int64_t)a.Hs * a.Ws * 3 : 0);  // (formed here, as it always was)
  s.src = img + ((int64_t)box.top * gm.Ws + box.left) * 3;
  s.rs = gm.Ws * 3;
  return s;
}

// The strip's sum of grey over the pixels as they stand before contrast -> work[sample][strip]. kP as in
// jitter_out_kernel: the same threads take the same pixels.
template <uint32_t kP, bool RAGGED>
__global__ __launch_bounds__(kT) void jitter_stats_kernel(const JitArgsT<RAGGED> ja) {
  extern __shared__ uint32_t tab[];  // [Wo] column taps, [rows] this strip's row taps
  __shared__ long long red[kT / 64];
  const RrcArgs& a = ja.r;
  const JitStrip s = jit_prologue<RAGGED>(ja, tab, false);
  const uint32_t rs = s.rs;
  const uint32_t Q = a.Wo / kP, Qc = Q < (uint32_t)kT ? Q : (uint32_t)kT, G = (uint32_t)kT / Qc;
  const uint32_t g = threadIdx.x / Qc, q0 = threadIdx.x - g * Qc;
  uint64_t sum = 0;  // <= rows * Wo * kJitT < 2^50
  if (s.ok && g < G) {  // (ok is uniform) an index outside the dataset reads nothing: its sums are zero
    for (uint32_t q = q0; q < Q; q += Qc) {
      uint32_t x0[kP], x1[kP];
      int32_t fx[kP];
#pragma unroll
      for (uint32_t k = 0; k < kP; ++k) {
        const uint32_t tx = tab[q * kP + k];
        x0[k] = (tx & 8191u) * 3;
        x1[k] = x0[k] + (tx >> 22) * 3;
        fx[k] = (int32_t)((tx >> 13) & 511u);
      }
      for (uint32_t il = g; il < s.nrow; il += G) {
        const uint32_t ty = tab[a.Wo + il];
        const uint32_t row0 = (ty & 8191u) * rs, row1 = row0 + (ty >> 22) * rs;
        const int32_t fy = (int32_t)((ty >> 13) & 511u);
#pragma unroll
        for (uint32_t k = 0; k < kP; ++k) {
          int32_t t[3];
          jit_pixel_pre(s.src, row0, row1, fy, x0[k], x1[k], fx[k], s.j, t);
          sum += (uint32_t)jit_grey(t);
        }
      }
    }
  }
  const long long w = wave_sum_i64((long long)sum);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long total = 0;
#pragma unroll
    for (int i = 0; i < kT / 64; ++i) total += red[i];
    ja.work[(int64_t)blockIdx.x * ja.strips + blockIdx.y] = (uint64_t)total;
  }
}

// resized_crop_kernel with the jitter between the blend and the normalisation. kP pixels per thread: 4 (Wo % 4
// == 0: the twelve floats stay inside the row, 16-byte aligned with X; written as three float4, which the
// compiler is free to regroup), or 1.
template <uint32_t kP, bool RAGGED>
__global__ __launch_bounds__(kT) void jitter_out_kernel(const JitArgsT<RAGGED> ja) {
  extern __shared__ uint32_t tab[];
  const RrcArgs& a = ja.r;
  const JitStrip s = jit_prologue<RAGGED>(ja, tab, true);
  const uint32_t WoC = a.Wo * 3, rs = s.rs, total = s.nrow * WoC;  // < 2^31 (host checks)
  float* __restrict__ out = a.X + ((int64_t)blockIdx.x * a.Ho + s.i0) * (int64_t)WoC;
  if (!s.ok) {  // (uniform) nothing to read: a zero image
    constexpr uint32_t kV = kP == 4 ? 4u : 1u;
    for (uint32_t e = threadIdx.x * kV; e < total; e += kT * kV) {
      if constexpr (kP == 4) {
        *reinterpret_cast<float4*>(out + e) = make_float4(0.f, 0.f, 0.f, 0.f);
      } else {
        out[e] = 0.f;
      }
    }
    return;
  }
  int32_t M = 0;  // the image's mean grey before contrast, from every strip's sum
  if (ja.work && jit_factor(s.j, kOpC) != kJitOne) {
    uint64_t sum = 0;
    const uint64_t* __restrict__ part = ja.work + (int64_t)blockIdx.x * ja.strips;
    for (uint32_t k = 0; k < ja.strips; ++k) sum += part[k];
    const uint64_t npx = (uint64_t)a.Ho * a.Wo;
    M = (int32_t)((sum + npx / 2) / npx);
  }
  const double sh0 = a.shift[0], sh1 = a.shift[1], sh2 = a.shift[2];
  const double sc0 = a.scale[0], sc1 = a.scale[1], sc2 = a.scale[2];
  const uint32_t Q = a.Wo / kP, Qc = Q < (uint32_t)kT ? Q : (uint32_t)kT, G = (uint32_t)kT / Qc;
  const uint32_t g = threadIdx.x / Qc, q0 = threadIdx.x - g * Qc;
  if (g >= G) return;
  for (uint32_t q = q0; q < Q; q += Qc) {
    uint32_t x0[kP], x1[kP];
    int32_t fx[kP];
#pragma unroll
    for (uint32_t k = 0; k < kP; ++k) {
      const uint32_t tx = tab[q * kP + k];
      x0[k] = (tx & 8191u) * 3;
      x1[k] = x0[k] + (tx >> 22) * 3;
      fx[k] = (int32_t)((tx >> 13) & 511u);
    }
    for (uint32_t il = g; il < s.nrow; il += G) {
      const uint32_t ty = tab[a.Wo + il];
      const uint32_t row0 = (ty & 8191u) * rs, row1 = row0 + (ty >> 22) * rs;
      const int32_t fy = (int32_t)((ty >> 13) & 511u);
      float v[3 * kP];
#pragma unroll
      for (uint32_t k = 0; k < kP; ++k) {
        int32_t t[3];
        jit_pixel_pre(s.src, row0, row1, fy, x0[k], x1[k], fx[k], s.j, t);
#pragma unroll
        for (uint32_t o = 0; o < 3; ++o)
          if (o >= s.j.cpos) jit_apply(s.j, o, M, t);
        v[3 * k + 0] = (float)(((double)t[0] - sh0) * sc0);
        v[3 * k + 1] = (float)(((double)t[1] - sh1) * sc1);
        v[3 * k + 2] = (float)(((double)t[2] - sh2) * sc2);
      }
      float* __restrict__ o = out + il * WoC + q * (3 * kP);
      if constexpr (kP == 4) {
        float4* __restrict__ o4 = reinterpret_cast<float4*>(o);
        o4[0] = make_float4(v[0], v[1], v[2], v[3]);
        o4[1] = make_float4(v[4], v[5], v[6], v[7]);
        o4[2] = make_float4(v[8], v[9], v[10], v[11]);
      } else {
        o[0] = v[0];
        o[1] = v[1];
        o[2] = v[2];
      }
    }
  }
}

bool jitter_range_ok(int32_t lo, int32_t hi) { return 0 <= lo && lo <= hi && hi <= 65536; }

// What the jitter adds to its plain launch's arguments. stats: whether the statistics pass runs.
struct JitHost {
  int32_t fb_lo, fb_hi, fc_lo, fc_hi, fs_lo, fs_hi;
  uint64_t* work;
  int64_t work_len;
  bool stats;
};

// The jitter's own refusals, made before its plain launch's. false: LBT_EINVAL.
bool jitter_own_ok(JitHost& j, int32_t B, int32_t C, int32_t Ho, int32_t augment) {
  if (C != 3) return false;
  if (!jitter_range_ok(j.fb_lo, j.fb_hi) || !jitter_range_ok(j.fc_lo, j.fc_hi) || !jitter_range_ok(j.fs_lo, j.fs_hi))
    return false;
  j.stats = augment != 0 && !(j.fc_lo == kJitOne && j.fc_hi == kJitOne);
  return !(j.stats && (B <= 0 || Ho <= 0 || Ho > 8192 || !j.work ||
                       j.work_len < lbt_batch_resized_crop_jitter_work(B, Ho)));
}

// The statistics pass (with contrast on) and the output pass, on the plain launch's packed arguments.
template <bool RAGGED>
int jitter_launch(const RrcArgsT<RAGGED>& r, const JitHost& j, int32_t B, void* stream) {
  JitArgsT<RAGGED> ja;
  ja.r = r;
  ja.fb_lo = (uint32_t)j.fb_lo; ja.fb_span = (uint32_t)(j.fb_hi - j.fb_lo + 1);
  ja.fc_lo = (uint32_t)j.fc_lo; ja.fc_span = (uint32_t)(j.fc_hi - j.fc_lo + 1);
  ja.fs_lo = (uint32_t)j.fs_lo; ja.fs_span = (uint32_t)(j.fs_hi - j.fs_lo + 1);
  ja.work = j.stats ? j.work : nullptr;
  const dim3 grid = rrc_grid(r, B);
  ja.strips = grid.y;
  const bool vec = r.Wo % 4 == 0 && (reinterpret_cast<uintptr_t>(r.X) & 15) == 0;
  const size_t lds = rrc_lds(r);
  hipStream_t st = (hipStream_t)stream;
  if (j.stats) {
    if (vec)
      hipLaunchKernelGGL((jitter_stats_kernel<4, RAGGED>), grid, dim3(kT), lds, st, ja);
    else
      hipLaunchKernelGGL((jitter_stats_kernel<1, RAGGED>), grid, dim3(kT), lds, st, ja);
    const int e = (int)hipGetLastError();
    if (e) return e;
  }
  if (vec)
    hipLaunchKernelGGL((jitter_out_kernel<4, RAGGED>), grid, dim3(kT), lds, st, ja);
  else
    hipLaunchKernelGGL((jitter_out_kernel<1, RAGGED>), grid, dim3(kT), lds, st, ja);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" int64_t lbt_batch_resized_crop_jitter_work(int32_t B, int32_t Ho) {
  if (B <= 0 || Ho <= 0 || Ho > 8192) return -1;
  const int32_t rows = rrc_strip_rows(B, Ho);
  return (int64_t)B * ((Ho + rows - 1) / rows);
}

extern "C" int lbt_batch_resized_crop_jitter(const uint8_t* data, const int32_t* labels, int64_t n_data,
                                             const int32_t* idx, int64_t first, float* X, int32_t* y, int32_t B,
                                             int32_t Hs, int32_t Ws, int32_t C, int32_t Ho, int32_t Wo, int32_t augment,
                                             int64_t a_lo, int64_t a_hi, const uint32_t* ratio_q16, int64_t q_lo,
                                             int64_t q_hi, int32_t ch, int32_t cw, const double* shift,
                                             const double* scale_c, int64_t base, uint64_t seed, uint64_t counter,
                                             int32_t fb_lo, int32_t fb_hi, int32_t fc_lo, int32_t fc_hi, int32_t fs_lo,
                                             int32_t fs_hi, uint64_t* work, int64_t work_len, void* stream) {
  JitHost j{fb_lo, fb_hi, fc_lo, fc_hi, fs_lo, fs_hi, work, work_len, false};
  RrcArgs a;
  if (!jitter_own_ok(j, B, C, Ho, augment) ||
      !rrc_pack(a, data, labels, n_data, idx, first, X, y, B, C, Ho, Wo, augment, ratio_q16, q_lo, q_hi, shift, scale_c,
                base, seed, counter) ||
      !rrc_pack_uniform(a, Hs, Ws, a_lo, a_hi, ch, cw))
    return LBT_EINVAL;
  // the validation transform: no jitter, the plain launch
  return augment ? jitter_launch<false>(a, j, B, stream) : rrc_launch<false>(a, B, stream);
}

extern "C" int lbt_batch_ragged_crop_jitter(const uint8_t* data, int64_t data_bytes, const lbt_image_geom* geom,
                                            const int32_t* labels, int64_t n_data, const int32_t* idx, int64_t first,
                                            float* X, int32_t* y, int32_t B, int32_t C, int32_t Ho, int32_t Wo,
                                            int32_t augment, const uint32_t* ratio_q16, int64_t q_lo, int64_t q_hi,
                                            const double* shift, const double* scale_c, int64_t base, uint64_t seed,
                                            uint64_t counter, int32_t fb_lo, int32_t fb_hi, int32_t fc_lo, int32_t fc_hi,
                                            int32_t fs_lo, int32_t fs_hi, uint64_t* work, int64_t work_len,
                                            void* stream) {
  JitHost j{fb_lo, fb_hi, fc_lo, fc_hi, fs_lo, fs_hi, work, work_len, false};
  RaggedArgs a;
  if (!jitter_own_ok(j, B, C, Ho, augment) ||
      !rrc_pack(a, data, labels, n_data, idx, first, X, y, B, C, Ho, Wo, augment, ratio_q16, q_lo, q_hi, shift, scale_c,
                base, seed, counter) ||
      !rrc_pack_ragged(a, geom, data_bytes))
    return LBT_EINVAL;
  return augment ? jitter_launch<true>(a, j, B, stream) : rrc_launch<true>(a, B, stream);
}
