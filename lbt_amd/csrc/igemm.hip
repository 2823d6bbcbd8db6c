// igemm.hip -- LDS-tiled int8 MFMA implicit GEMM for the wide layers (ResNet-50 shapes, SURVEY 8(f)
// rank 1): channel counts that are multiples of 64 on the gathered side and of 16 on the output
// side, any count (conv_mfma.hip's register-resident kernels take <= 128 channels).
//
//   fwd   : y[m = (n,oh,ow)][co] = sum_{tap,ci} x[n, oh*S+kh-P, ow*S+kw-P, ci] * W[tap][ci][co]
//   dgrad : dx[m = (n,ih,iw)][ci] = sum_{tap,co} g[n, (ih+P-kh)/S, (iw+P-kw)/S, co] * W[tap][ci][co]
//                                   (taps whose position is not an output pixel contribute 0)
// B = the packed weight image of lbt_dfxp_quantize_weight ([col][k], k = (tap, 16-channel slice)).
//
// Workgroup tile 128 rows x 128 columns, 4 waves of 64 x 64 (4 x 4 v_mfma_i32_16x16x64_i8 tiles),
// k-blocks of 64 = one tap x 64 channels; operands staged through double-buffered LDS: the next
// k-block's global loads are in flight while the current one is multiplied.
//
// A16: the gathered operand is int16 codes (9..16-bit: the signed 9-bit image of a Conv2d_q input
// or 16-bit gradient codes, config 4). Each code is split a = 256*hi + lo' + 128 with hi, lo' int8,
// so sum a*w = 256 sum hi*w + sum lo'*w + 128 sum w: two int8 MFMA passes, plus one against an
// all-ones A fragment for sum_k w per column; combined exactly in int64 in the epilogue. Positions
// outside the image (a = 0) are (hi, lo') = (0, -128), which the identity keeps exact.
// A8: int8 codes, either signed (fill 0) or offset-by-128 ("u8off", fill -128, + 128 sum_k w).
//
// This unit: the 64 / 128-row kernel, split-K, the parity classes of a strided dgrad and the forward /
// dgrad entry points. The 256-row kernels are igemm_big.hip and igemm_persist.hip, the weight gradients
// igemm_wgrad.hip; igemm.h is what they share.
#include "igemm.h"

#include <type_traits>

namespace {

constexpr int kBM = 128, kBN = 128;
constexpr int kRow = kBK + 16;  // LDS row stride in bytes (16-byte pad staggers the banks)

// every tap, rows = every output pixel (fwd, unit-stride dgrad)
void all_taps(IgArgs& p, int mode) {
  const lbt_conv_desc& d = p.d;
  p.nkh = d.KH; p.nkw = d.KW; p.kh0 = 0; p.kw0 = 0;
  p.oy = d.PT; p.ox = d.PL;
  p.ch = mode == MODE_FWD ? d.Ho : d.H;
  p.cw = mode == MODE_FWD ? d.Wo : d.W;
  p.cpy = 0; p.cpx = 0;
}

// BM x BN workgroup tile (64 or 128 each), 2 x 2 waves of (BM/2) x (BN/2): MI x NJ MFMA tiles
template <int MODE, bool A16, bool ADD, int BM, int BN, int D, bool CLS>
__global__ __launch_bounds__(kT) void igemm_kernel(IgArgs p) {
  constexpr int NA = A16 ? 2 : 1;  // A tiles per k-block: (hi, lo') or one
  constexpr int HA = BM / 64, HB = BN / 64;  // 64-row loader passes of A / B
  constexpr int MI = BM / 32, NJ = BN / 32;  // 16x16 tiles per wave
  __shared__ __attribute__((aligned(16))) int8_t sA[2][NA][BM * kRow];
  __shared__ __attribute__((aligned(16))) int8_t sB[2][BN * kRow];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int64_t m0 = (int64_t)blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  const lbt_conv_desc& d = p.d;
  const int OH = p.ch, OW = p.cw;  // the row grid (dgrad parity class: its ch x cw pixels)
  const int SH = MODE == MODE_FWD ? d.H : d.Ho, SW = MODE == MODE_FWD ? d.W : d.Wo;
  const int cblocks = p.cred / kBK, nk_all = p.nkh * p.nkw * cblocks;
  const int nk = nk_all / p.ksplit, kbase = (int)blockIdx.z * nk;  // this split's k-blocks

  // ---- loader roles: A rows (t >> 2) and (t >> 2) + 64, 16-byte segment (t & 3) of the 64 channels
  // (A16: 32-byte segments = 16 codes); B columns likewise
  const int lr = t >> 2, seg = t & 3;
  int an[HA], ay[HA], ax[HA];
  bool arow[HA];
#pragma unroll
  for (int h = 0; h < HA; ++h) {
    const int64_t m = m0 + lr + 64 * h;
    arow[h] = m < p.M;
    const uint32_t mu = (uint32_t)(arow[h] ? m : 0);
    ax[h] = (int)(mu % (uint32_t)OW);
    const uint32_t tt = mu / (uint32_t)OW;
    ay[h] = (int)(tt % (uint32_t)OH);
    an[h] = (int)(tt / (uint32_t)OH);
  }
  // global -> register stage of one k-block
  // D register stages: the global loads of k-block b land in stage b % D, D k-blocks ahead of use
  v4i ra[D][HA][A16 ? 2 : 1], rb[D][HB];
  bool rv[D][HA];
  auto load_k = [&](int kbl, int st) {
    const int kb = kbase + kbl;
    const int tap = kb / cblocks, cb = kb - tap * cblocks;
    const int th = tap / p.nkw, tw = tap - th * p.nkw;
    const int kh = MODE == MODE_FWD ? th : p.kh0 + d.SH * th, kw = MODE == MODE_FWD ? tw : p.kw0 + d.SW * tw;
    const int kbw = (kh * d.KW + kw) * cblocks + cb;  // the weight image's k-block
#pragma unroll
    for (int h = 0; h < HA; ++h) {
      int sy, sx;
      if (MODE == MODE_FWD) {
        sy = ay[h] * d.SH + kh - d.PT;
        sx = ax[h] * d.SW + kw - d.PL;
      } else {  // ih = yc * SH + cpy: (ih + PT - kh) / SH = yc + oy - th exactly
        sy = ay[h] + p.oy - th;
        sx = ax[h] + p.ox - tw;
      }
      const bool ok = (unsigned)sy < (unsigned)SH && (unsigned)sx < (unsigned)SW && arow[h];
      rv[st][h] = ok;
      // 32-bit element offsets (launcher: every operand < 2^31 elements)
      const uint32_t pix = ok ? (uint32_t)((an[h] * SH + sy) * SW + sx) : 0u;
      if constexpr (A16) {
        const int16_t* src = reinterpret_cast<const int16_t*>(p.a) + (pix * (uint32_t)p.cred + (uint32_t)(cb * kBK + seg * 16));
        ra[st][h][0] = *reinterpret_cast<const v4i*>(src);
        ra[st][h][1] = *reinterpret_cast<const v4i*>(src + 8);
      } else {
        const int8_t* src = reinterpret_cast<const int8_t*>(p.a) + (pix * (uint32_t)p.cred + (uint32_t)(cb * kBK + seg * 16));
        ra[st][h][0] = *reinterpret_cast<const v4i*>(src);
      }
    }
#pragma unroll
    for (int h = 0; h < HB; ++h) {
      const int col = n0 + lr + 64 * h;
      const int colc = col < p.ncol ? col : 0;
      rb[st][h] = *reinterpret_cast<const v4i*>(p.b + ((uint32_t)(colc * p.ks + kbw * 4 + seg) << 4));
      if (col >= p.ncol) rb[st][h] = v4i{0, 0, 0, 0};
    }
  };
  auto store_k = [&](int buf, int st) {
#pragma unroll
    for (int h = 0; h < HA; ++h) {
      const int row = lr + 64 * h;
      if constexpr (A16) {
        // 16 codes -> 16 hi bytes and 16 lo' bytes (a = 256 hi + lo' + 128); outside: (0, -128)
        int hi[4], lo[4];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const uint32_t c01 = (uint32_t)ra[st][h][w >> 1][(w & 1) * 2], c23 = (uint32_t)ra[st][h][w >> 1][(w & 1) * 2 + 1];
          // codes (int16) e0 e1 | e2 e3; hi = arithmetic >> 8 (the high byte), lo' = low byte ^ 0x80
          hi[w] = (int)__builtin_amdgcn_perm(c23, c01, 0x07050301u);
          lo[w] = (int)(__builtin_amdgcn_perm(c23, c01, 0x06040200u) ^ 0x80808080u);
          if (!rv[st][h]) { hi[w] = 0; lo[w] = (int)0x80808080u; }
        }
        *reinterpret_cast<v4i*>(&sA[buf][0][row * kRow + seg * 16]) = v4i{hi[0], hi[1], hi[2], hi[3]};
        *reinterpret_cast<v4i*>(&sA[buf][1][row * kRow + seg * 16]) = v4i{lo[0], lo[1], lo[2], lo[3]};
      } else {
        const int fill = p.a_u8off ? (int)0x80808080u : 0;
        v4i v = ra[st][h][0];
        if (!rv[st][h]) v = v4i{fill, fill, fill, fill};
        *reinterpret_cast<v4i*>(&sA[buf][0][row * kRow + seg * 16]) = v;
      }
    }
#pragma unroll
    for (int h = 0; h < HB; ++h) *reinterpret_cast<v4i*>(&sB[buf][(lr + 64 * h) * kRow + seg * 16]) = rb[st][h];
  };

  v4i acc[NA][MI][NJ], accw[NJ];
#pragma unroll
  for (int a = 0; a < NA; ++a)
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[a][i][j] = v4i{0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < NJ; ++j) accw[j] = v4i{0, 0, 0, 0};
  const v4i ones = v4i{0x01010101, 0x01010101, 0x01010101, 0x01010101};
  const bool want_w = A16 || p.a_u8off;  // sum_k W per column (the +128 term)

  // prologue: block 0 into LDS[0], blocks 1 .. D in flight (stage b % D). nk % D == 0 (launcher) and
  // every load / store below is unconditional (block indices clamped, a stale store into the buffer
  // nobody reads any more is harmless): straight-line code, so the compiler's wait counts let the
  // younger stages stay in flight instead of draining them (vmcnt(0)) at every branch
  load_k(0, 0);
  store_k(0, 0);
#pragma unroll
  for (int b = 1; b <= D; ++b) load_k(b < nk ? b : nk - 1, b % D);
  __syncthreads();
  const int r = lane & 15, q = lane >> 4;
  for (int kb0 = 0; kb0 < nk; kb0 += D) {
#pragma unroll
    for (int u = 0; u < D; ++u) {  // kb0 % D == 0: stage indices below are compile-time
      const int kb = kb0 + u;
      const int cur = kb & 1;
      v4i bf[NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        bf[j] = *reinterpret_cast<const v4i*>(&sB[cur][(wn * (BN / 2) + j * 16 + r) * kRow + q * 16]);
#pragma unroll
      for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int i = 0; i < MI; ++i) {
          const v4i af = *reinterpret_cast<const v4i*>(&sA[cur][a][(wm * (BM / 2) + i * 16 + r) * kRow + q * 16]);
#pragma unroll
          for (int j = 0; j < NJ; ++j)
            acc[a][i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af, bf[j], acc[a][i][j], 0, 0, 0);
        }
      if (want_w) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) accw[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, bf[j], accw[j], 0, 0, 0);
      }
      const int st = (u + 1) % D;  // block kb + 1's stage
      store_k(cur ^ 1, st);  // the other buffer: its readers finished before the last barrier
      load_k(kb + 1 + D < nk ? kb + 1 + D : nk - 1, st);
      __syncthreads();
    }
  }

  // ---- epilogue: lane owns column (tile col + r), rows (tile row + 4q + e). Index math kept
  // off the per-element path: one 64-bit base per column tile, 32-bit row offsets, row checks only
  // on the last (ragged) tile; A8 sums fit int32 (launcher: K * 255 * 128 < 2^31), A16 sums are
  // formed exactly in double (|s| < 2^53) and rounded once to fp32 -- the same value as
  // (float)(int64) s.
  const float scale = ldexpf(1.0f, -(frac_exp(p.qa) + frac_exp(p.qb)));
  constexpr bool addv = MODE == MODE_DGRAD && ADD;
  const int ncol = p.ncol;
  const int64_t rtile = m0 + wm * (BM / 2) + q * 4;  // + i * 16 + e
  const bool full = m0 + BM <= p.M;
  const int rlim = full ? (BM / 2) : (int)(p.M - rtile);  // rows (i * 16 + e) < rlim are real
  const int u8 = p.a_u8off ? 128 : 0;
  if (p.ksplit > 1) {  // uniform: store this split's exact partials
    const int64_t plane = p.M * ncol;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int ctile = n0 + wn * (BN / 2) + j * 16;
      if (ctile >= ncol) continue;
      const int wsum = want_w ? accw[j][0] : 0;
      int32_t* pp = p.part + (int64_t)blockIdx.z * (A16 ? 2 : 1) * plane + rtile * ncol + ctile + r;
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (!(full || i * 16 + e < rlim)) continue;
          if constexpr (A16) {
            pp[(i * 16 + e) * ncol] = acc[0][i][j][e];
            pp[plane + (i * 16 + e) * ncol] = acc[1][i][j][e] + 128 * wsum;
          } else {
            pp[(i * 16 + e) * ncol] = acc[0][i][j][e] + u8 * wsum;
          }
        }
    }
    return;
  }
  if constexpr (MODE == MODE_FWD && !A16) {
    if (p.yq) {  // uniform: quantising epilogue
      quant_epilogue<MI, NJ>(p, acc[0], accw, want_w ? u8 : 0, scale, rtile, rlim, full, n0 + wn * (BN / 2), r, q);
      return;
    }
  }
  if constexpr (CLS) {  // parity-class rows: each row's dx pixel, 32-bit (launcher: dx < 2^31 elements)
    uint32_t roff[MI][4];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t m = rtile + i * 16 + e;
        const uint32_t mu = (uint32_t)(m < p.M ? m : 0);
        const uint32_t xc = mu % (uint32_t)p.cw, t2 = mu / (uint32_t)p.cw;
        const uint32_t yc = t2 % (uint32_t)p.ch, n = t2 / (uint32_t)p.ch;
        roff[i][e] = ((n * (uint32_t)d.H + yc * (uint32_t)d.SH + (uint32_t)p.cpy) * (uint32_t)d.W +
                      xc * (uint32_t)d.SW + (uint32_t)p.cpx) * (uint32_t)ncol;
      }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int ctile = n0 + wn * (BN / 2) + j * 16;
      if (ctile >= ncol) continue;
      const uint32_t col = (uint32_t)(ctile + r);
      const int wsum = want_w ? accw[j][0] : 0;
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (!(full || i * 16 + e < rlim)) continue;
          float v;
          if constexpr (A16) {
            const double hs = (double)acc[0][i][j][e] * 256.0;
            const double ls = (double)(acc[1][i][j][e] + 128 * wsum);
            v = (float)(hs + ls) * scale;
          } else {
            v = (float)(acc[0][i][j][e] + u8 * wsum) * scale;
          }
          if constexpr (addv) v = v + p.add_src[roff[i][e] + col];
          p.y[roff[i][e] + col] = v;
        }
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int ctile = n0 + wn * (BN / 2) + j * 16;
    if (ctile >= ncol) continue;  // uniform: ncol % 16 == 0
    const int col = ctile + r;
    float* yp = p.y + rtile * ncol + col;
    const float* ap = addv ? p.add_src + rtile * ncol + col : nullptr;
    float av[MI][4];
    if constexpr (addv) {
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) av[i][e] = (i * 16 + e < rlim) ? ap[(i * 16 + e) * ncol] : 0.f;
    }
    const int wsum = want_w ? accw[j][0] : 0;  // every row of accw holds sum_k W[col][k]
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v;
        if constexpr (A16) {
          const double hs = (double)acc[0][i][j][e] * 256.0;  // exact
          const double ls = (double)(acc[1][i][j][e] + 128 * wsum);  // |.| < 2^31: K * 255 * 128 bound
          v = (float)(hs + ls) * scale;  // hs + ls exact (< 2^53): one rounding, as (float)(int64)
        } else {
          v = (float)(acc[0][i][j][e] + u8 * wsum) * scale;
        }
        if (full || i * 16 + e < rlim) yp[(i * 16 + e) * ncol] = addv ? v + av[i][e] : v;
      }
  }
}

// Sum of the split partials + the epilogue of igemm_kernel, element-wise (4 per thread).
template <bool A16, bool ADD>
__global__ __launch_bounds__(256) void igemm_splitk_reduce_kernel(IgArgs p) {
  const int64_t plane = p.M * p.ncol;
  const int64_t i4 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i4 >= plane) return;
  const float scale = ldexpf(1.0f, -(frac_exp(p.qa) + frac_exp(p.qb)));
  int4 s0 = make_int4(0, 0, 0, 0), s1 = make_int4(0, 0, 0, 0);
  for (int z = 0; z < p.ksplit; ++z) {
    const int4 a = *reinterpret_cast<const int4*>(p.part + (int64_t)z * (A16 ? 2 : 1) * plane + i4);
    s0.x += a.x; s0.y += a.y; s0.z += a.z; s0.w += a.w;
    if constexpr (A16) {
      const int4 b = *reinterpret_cast<const int4*>(p.part + ((int64_t)z * 2 + 1) * plane + i4);
      s1.x += b.x; s1.y += b.y; s1.z += b.z; s1.w += b.w;
    }
  }
  const int h[4] = {s0.x, s0.y, s0.z, s0.w}, l[4] = {s1.x, s1.y, s1.z, s1.w};
  float v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if constexpr (A16)
      v[k] = (float)((double)h[k] * 256.0 + (double)l[k]) * scale;  // exact sum, one rounding
    else
      v[k] = (float)h[k] * scale;
  }
  if constexpr (ADD) {
    const float4 a = *reinterpret_cast<const float4*>(p.add_src + i4);
    v[0] = v[0] + a.x; v[1] = v[1] + a.y; v[2] = v[2] + a.z; v[3] = v[3] + a.w;
  }
  *reinterpret_cast<float4*>(p.y + i4) = make_float4(v[0], v[1], v[2], v[3]);
}

template <int MODE, bool A16, int BM, int BN, bool CLS = false>
void launch_tile(const IgArgs& p, hipStream_t st) {
  const dim3 grid((unsigned)((p.M + BM - 1) / BM), (unsigned)((p.ncol + BN - 1) / BN), (unsigned)p.ksplit);
  // register stages in flight: a divisor of the split's k-block count (3x3 convs: 9 * Cin/64 -> 3;
  // 1x1: 2), 1 for the VGPR-heavy 128x128 tiles
  const int nk = p.nkh * p.nkw * (p.cred / kBK) / p.ksplit;
  const int D = (BM == 128 && BN == 128) ? 1 : (nk % 3 == 0 && !CLS ? 3 : (nk % 2 == 0 ? 2 : 1));
#define LBT_IG(DD)                                                                      \
  do {                                                                                  \
    if (MODE == MODE_DGRAD && p.add_src)                                                \
      hipLaunchKernelGGL((igemm_kernel<MODE, A16, true, BM, BN, DD, CLS>), grid, dim3(kT), 0, st, p);  \
    else                                                                                \
      hipLaunchKernelGGL((igemm_kernel<MODE, A16, false, BM, BN, DD, CLS>), grid, dim3(kT), 0, st, p); \
  } while (0)
  if constexpr (CLS) {
    if (D == 2) LBT_IG(2); else LBT_IG(1);
  } else {
    if (D == 3) LBT_IG(3); else if (D == 2) LBT_IG(2); else LBT_IG(1);
  }
#undef LBT_IG
  if (p.ksplit > 1) {
    const dim3 g2((unsigned)((p.M * p.ncol / 4 + 255) / 256));
    if (MODE == MODE_DGRAD && p.add_src)
      hipLaunchKernelGGL((igemm_splitk_reduce_kernel<A16, true>), g2, dim3(256), 0, st, p);
    else
      hipLaunchKernelGGL((igemm_splitk_reduce_kernel<A16, false>), g2, dim3(256), 0, st, p);
  }
}

// Split-K factor: when even 64 x 64-row tiles leave the chip with fewer than ~2 workgroups per CU
// and the k loop is long, the smallest divisor of the k-block count that reaches ~512 workgroups
// (each split keeping >= 4 k-blocks). 1 = no split.
int choose_ksplit(int64_t M, int ncol, int nk) {
  const int64_t tiles = ((M + 63) / 64) * ((ncol + 127) / 128);
  if (tiles >= 256 || nk < 8 || getenv_int("LBT_IGEMM_SPLITK", 1) == 0) return 1;
  static const int cand[] = {2, 3, 4, 6, 8, 9, 12, 16};
  int best = 1;
  for (int c : cand) {
    if (nk % c || nk / c < 4) continue;
    best = c;
    if (tiles * c >= 512) break;
  }
  return best;
}

// workspace bytes a split launch needs (0: none)
int64_t splitk_bytes(int64_t M, int ncol, int nk, bool a16) {
  const int ks = choose_ksplit(M, ncol, nk);
  return ks > 1 ? (int64_t)ks * (a16 ? 2 : 1) * M * ncol * 4 : 0;
}

// Tile choice: 64 columns when the GEMM has <= 64 (no MFMAs on padding columns), and 64 rows
// when 128-row tiles would leave the 256 CUs without two workgroups each.
template <int MODE, bool A16, bool CLS = false>
int launch(const IgArgs& p, hipStream_t st) {
  const int64_t mb = (p.M + kBM - 1) / kBM;
  if (mb > 0x7fffffff / 2 || (p.ncol + 63) / 64 > 65535) return LBT_EINVAL;
  const bool bn64 = p.ncol <= 64 || getenv_int("LBT_IGEMM_BN", 128) == 64;
  if constexpr (CLS) {  // parity classes of a strided dgrad: 64-row tiles only (fewer variants)
    if (bn64) launch_tile<MODE, A16, 64, 64, true>(p, st); else launch_tile<MODE, A16, 64, 128, true>(p, st);
    return (int)hipGetLastError();
  }
  if (igemm_launch_big(MODE, A16, p, st)) return (int)hipGetLastError();
  const int64_t nb = (p.ncol + (bn64 ? 63 : 127)) / (bn64 ? 64 : 128);
  // ... and always for 16-bit codes when the tile would be 128 x 128: that variant needs 256 VGPRs
  // (one wave per SIMD), which leaves its fp32 epilogue stores unhidden
  const bool bm64 = mb * nb < getenv_int("LBT_IGEMM_MIN_WG", 512) || (A16 && !bn64) || p.ksplit > 1;
  if (bm64) {
    if (bn64) launch_tile<MODE, A16, 64, 64>(p, st); else launch_tile<MODE, A16, 64, 128>(p, st);
  } else {
    if (bn64) launch_tile<MODE, A16, 128, 64>(p, st); else launch_tile<MODE, A16, 128, 128>(p, st);
  }
  return (int)hipGetLastError();
}

// dx of a parity class no tap reaches (a 1x1 stride-2 conv's odd pixels): add_src, or 0
__global__ __launch_bounds__(256) void dgrad_fill_class_kernel(IgArgs p) {
  const int64_t i4 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i4 >= p.M * p.ncol) return;
  const int64_t m = i4 / p.ncol;
  const int c = (int)(i4 - m * p.ncol);
  const lbt_conv_desc& d = p.d;
  const int64_t xc = m % p.cw, t2 = m / p.cw, yc = t2 % p.ch, n = t2 / p.ch;
  const int64_t off = ((n * d.H + yc * d.SH + p.cpy) * d.W + xc * d.SW + p.cpx) * p.ncol + c;
  *reinterpret_cast<float4*>(p.y + off) =
      p.add_src ? *reinterpret_cast<const float4*>(p.add_src + off) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// Strided dgrad as SH x SW parity-class GEMMs (IgArgs: nkh ...): each class runs only the taps that
// reach it, so no MFMA multiplies the zero rows of the stride's implicit upsampling. Never split.
template <bool A16>
int dgrad_classes(IgArgs p, hipStream_t st) {
  const lbt_conv_desc& d = p.d;
  if ((int64_t)d.N * d.H * d.W * d.Cin >= ((int64_t)1 << 31)) return LBT_EINVAL;  // 32-bit row offsets
  p.ksplit = 1;
  for (int py = 0; py < d.SH; ++py)
    for (int px = 0; px < d.SW; ++px) {
      const int ch = py < d.H ? (d.H - py + d.SH - 1) / d.SH : 0;
      const int cw = px < d.W ? (d.W - px + d.SW - 1) / d.SW : 0;
      if (!ch || !cw) continue;
      const int kh0 = (py + d.PT) % d.SH, kw0 = (px + d.PL) % d.SW;
      p.nkh = kh0 < d.KH ? (d.KH - kh0 + d.SH - 1) / d.SH : 0;
      p.nkw = kw0 < d.KW ? (d.KW - kw0 + d.SW - 1) / d.SW : 0;
      p.kh0 = kh0; p.kw0 = kw0;
      p.oy = (py + d.PT - kh0) / d.SH; p.ox = (px + d.PL - kw0) / d.SW;
      p.cpy = py; p.cpx = px; p.ch = ch; p.cw = cw;
      p.M = (int64_t)d.N * ch * cw;
      int rc;
      if (!p.nkh || !p.nkw) {
        hipLaunchKernelGGL(dgrad_fill_class_kernel, dim3((unsigned)((p.M * p.ncol / 4 + 255) / 256)), dim3(256), 0, st,
                           p);
        rc = (int)hipGetLastError();
      } else {
        rc = launch<MODE_DGRAD, A16, true>(p, st);
      }
      if (rc) return rc;
    }
  return 0;
}

// ---------------------------------------------------------------------------- entry points
// The shape checks and the IgArgs fill of the forward entry points (lbt_conv_fwd_igemm, _q, _ws); false =
// the shape does not qualify. They differ in
//   mn_bits      M * ncol < 2^mn_bits: 40 in lbt_conv_fwd_igemm, 31 in _q and _ws
//   colsum, y    _q has neither (its outputs are yq / chsum)
// and, outside this function, in their pointer checks, in _q refusing 16-bit codes and qout.bits outside
// 2..8, in ksplit / part (_ws) and in perm / npb (_q).
bool fwd_args(IgArgs& p, const void* xq, int a_kind, const int8_t* wf, int ksf, const int32_t* colsum,
              const lbt_conv_desc& d, const lbt_qdesc& qx, const lbt_qdesc& qw, float* y, int mn_bits) {
  if (!desc_ok(d) || d.Cin % kBK || d.Cout % 16) return false;
  if ((int64_t)d.KH * d.KW * d.Cin * 255 * 128 >= ((int64_t)1 << 31)) return false;  // int32 epilogue sums
  if ((int64_t)d.N * d.H * d.W * d.Cin >= ((int64_t)1 << 31) || (int64_t)ksf * 16 * d.Cout >= ((int64_t)1 << 31))
    return false;  // 32-bit operand offsets
  if (ksf * 16 < d.KH * d.KW * d.Cin) return false;
  p = IgArgs{};
  p.a = xq; p.b = wf; p.ks = ksf; p.cred = d.Cin; p.a_u8off = a_kind == 1; p.d = d; p.qa = qx; p.qb = qw;
  p.colsum = colsum; p.y = y; p.add_src = nullptr; p.M = (int64_t)d.N * d.Ho * d.Wo; p.ncol = d.Cout;
  if (p.M * p.ncol >= ((int64_t)1 << mn_bits)) return false;
  p.ksplit = 1;
  all_taps(p, MODE_FWD);
  return true;
}

// The same for dgrad (lbt_conv_dgrad_igemm, _ws, and the fused branch of _bna / _bn3, which has no dx):
//   mn_bits      0: no bound on M * ncol (lbt_conv_dgrad_igemm); 31 in _ws and the fused branch
bool dgrad_args(IgArgs& p, const void* gq, const int8_t* wd, int ksd, const lbt_conv_desc& d, const lbt_qdesc& qg,
                const lbt_qdesc& qw, float* dx, const float* add_src, int mn_bits) {
  if (!desc_ok(d) || d.Cout % kBK || d.Cin % 16) return false;
  if ((int64_t)d.KH * d.KW * d.Cout * 255 * 128 >= ((int64_t)1 << 31)) return false;  // int32 epilogue sums
  if ((int64_t)d.N * d.Ho * d.Wo * d.Cout >= ((int64_t)1 << 31) || (int64_t)ksd * 16 * d.Cin >= ((int64_t)1 << 31))
    return false;  // 32-bit operand offsets
  if (ksd * 16 < d.KH * d.KW * d.Cout) return false;
  p = IgArgs{};
  p.a = gq; p.b = wd; p.ks = ksd; p.cred = d.Cout; p.a_u8off = 0; p.d = d; p.qa = qg; p.qb = qw;
  p.colsum = nullptr; p.y = dx; p.add_src = add_src; p.M = (int64_t)d.N * d.H * d.W; p.ncol = d.Cin;
  if (mn_bits && p.M * p.ncol >= ((int64_t)1 << mn_bits)) return false;
  p.ksplit = 1;
  all_taps(p, MODE_DGRAD);
  return true;
}

// The fused branch of lbt_conv_dgrad_igemm_bna / _bn3 (16-bit codes, the pass-A epilogue of the 256-row
// kernel instead of dx) asks more than dgrad_args: unit stride, Cin % 64 and a GEMM that does not split
// (no workspace). false is not an error here: the caller takes its unfused path.
bool dgrad_fused_args(IgArgs& p, const int16_t* gq, const int8_t* wd, int ksd, const lbt_conv_desc& d,
                      const lbt_qdesc& qg, const lbt_qdesc& qw) {
  if (d.SH != 1 || d.SW != 1 || d.Cin % 64) return false;
  if (!dgrad_args(p, gq, wd, ksd, d, qg, qw, nullptr, nullptr, 31)) return false;
  if (lbt_igemm_workspace_bytes(d, 1, 1) != 0) return false;
  p.npb = (d.H * d.W + 15) / 16;  // sample-blocked row tiles
  return true;
}

int fwd_launch(const IgArgs& p, int a_kind, hipStream_t st) {
  return a_kind == 2 ? launch<MODE_FWD, true>(p, st) : launch<MODE_FWD, false>(p, st);
}

int dgrad_launch(const IgArgs& p, bool g_i16, hipStream_t st) {
  if (p.d.SH > 1 || p.d.SW > 1) return g_i16 ? dgrad_classes<true>(p, st) : dgrad_classes<false>(p, st);
  return g_i16 ? launch<MODE_DGRAD, true>(p, st) : launch<MODE_DGRAD, false>(p, st);
}

}  // namespace

// a_kind: 0 int8 signed, 1 int8 offset (q - 128; needs colsum = sum_k W per output channel), 2 int16
extern "C" int lbt_conv_fwd_igemm(const void* xq, int32_t a_kind, const int8_t* wf, int32_t ksf,
                                  const int32_t* colsum, lbt_conv_desc d, lbt_qdesc qx, lbt_qdesc qw, float* y,
                                  void* stream) {
  IgArgs p;
  if (!y || !wf || !fwd_args(p, xq, a_kind, wf, ksf, colsum, d, qx, qw, y, 40)) return LBT_EINVAL;
  return fwd_launch(p, a_kind, (hipStream_t)stream);
}

// Forward whose epilogue is the consuming Normalization_q's input quantiser (no fp32 y): int8 codes
// yq + qout's overflow counters + exact channel sums chsum[NSHARD][2 * Cout]. A8 codes only (a_kind
// 0 / 1); never split (short-M GEMMs use lbt_conv_fwd_igemm_ws + lbt_dfxp_quantize).
extern "C" int lbt_conv_fwd_igemm_q(const void* xq, int32_t a_kind, const int8_t* wf, int32_t ksf, lbt_conv_desc d,
                                    lbt_qdesc qx, lbt_qdesc qw, int8_t* yq, lbt_qdesc qout, int64_t* chsum,
                                    void* stream) {
  IgArgs p;
  if (!yq || !wf || !chsum || a_kind == 2 || qout.bits < 2 || qout.bits > 8) return LBT_EINVAL;
  if (!fwd_args(p, xq, a_kind, wf, ksf, nullptr, d, qx, qw, nullptr, 31)) return LBT_EINVAL;
  p.yq = yq; p.qout = qout; p.chsum = chsum; p.hw = d.Ho * d.Wo;
  // the 256-row kernels' quantising epilogue on sample-blocked tiles (1: quantq_epilogue, >= 2: the
  // persistent igemm_fwdq_kernel where it applies)
  p.perm = igemm_fwdq_perm() > 0 ? igemm_fwdq_perm() : 0;
  p.npb = (d.Ho * d.Wo + 15) / 16;
  return launch<MODE_FWD, false>(p, (hipStream_t)stream);
}

// Workspace of the split-K variants below (0: that GEMM does not split). mode 0 fwd, 1 dgrad.
extern "C" int64_t lbt_igemm_workspace_bytes(lbt_conv_desc d, int32_t mode, int32_t a16) {
  if (!desc_ok(d)) return 0;
  if (mode == 0)
    return splitk_bytes((int64_t)d.N * d.Ho * d.Wo, d.Cout, d.KH * d.KW * (d.Cin / kBK), a16 != 0);
  if (d.SH > 1 || d.SW > 1) return 0;  // strided dgrad: parity classes, never split
  return splitk_bytes((int64_t)d.N * d.H * d.W, d.Cin, d.KH * d.KW * (d.Cout / kBK), a16 != 0);
}

// lbt_conv_fwd_igemm with a caller-owned workspace (ws_bytes >= lbt_igemm_workspace_bytes): the
// short-M / long-K GEMMs split K over workgroups, exact int32 partials, one reduce launch after.
extern "C" int lbt_conv_fwd_igemm_ws(const void* xq, int32_t a_kind, const int8_t* wf, int32_t ksf,
                                     const int32_t* colsum, lbt_conv_desc d, lbt_qdesc qx, lbt_qdesc qw, float* y,
                                     void* ws, int64_t ws_bytes, void* stream) {
  IgArgs p;
  if (!y || !wf || !fwd_args(p, xq, a_kind, wf, ksf, colsum, d, qx, qw, y, 31)) return LBT_EINVAL;
  const int64_t need = lbt_igemm_workspace_bytes(d, 0, a_kind == 2);
  p.ksplit = (need > 0 && ws && ws_bytes >= need) ? choose_ksplit(p.M, p.ncol, d.KH * d.KW * (d.Cin / kBK)) : 1;
  p.part = reinterpret_cast<int32_t*>(ws);
  return fwd_launch(p, a_kind, (hipStream_t)stream);
}

// g_i16: gradient codes are int16 (9..16-bit) instead of int8
extern "C" int lbt_conv_dgrad_igemm(const void* gq, int32_t g_i16, const int8_t* wd, int32_t ksd, lbt_conv_desc d,
                                    lbt_qdesc qg, lbt_qdesc qw, float* dx, const float* add_src, void* stream) {
  IgArgs p;
  if (!dx || !wd || !dgrad_args(p, gq, wd, ksd, d, qg, qw, dx, add_src, 0)) return LBT_EINVAL;
  return dgrad_launch(p, g_i16 != 0, (hipStream_t)stream);
}

extern "C" int lbt_conv_dgrad_igemm_ws(const void* gq, int32_t g_i16, const int8_t* wd, int32_t ksd, lbt_conv_desc d,
                                       lbt_qdesc qg, lbt_qdesc qw, float* dx, const float* add_src, void* ws,
                                       int64_t ws_bytes, void* stream) {
  IgArgs p;
  if (!dx || !wd || !dgrad_args(p, gq, wd, ksd, d, qg, qw, dx, add_src, 31)) return LBT_EINVAL;
  const int64_t need = lbt_igemm_workspace_bytes(d, 1, g_i16);
  p.ksplit = (need > 0 && ws && ws_bytes >= need) ? choose_ksplit(p.M, p.ncol, d.KH * d.KW * (d.Cout / kBK)) : 1;
  p.part = reinterpret_cast<int32_t*>(ws);
  return dgrad_launch(p, g_i16 != 0, (hipStream_t)stream);
}

// The dgrad with the mask_r BN pass A it feeds (include/lbt_dfxp.h lbt_dgrad_bna): in the 256-row
// kernel's epilogue when that kernel takes the GEMM, else dgrad into dx + lbt_bn_bwd_a_wide_masked.
// LBT_DGRAD_BNA=0: always the second form (A/B).
extern "C" int lbt_conv_dgrad_igemm_bna(const int16_t* gq, const int8_t* wd, int32_t ksd, lbt_conv_desc d,
                                        lbt_qdesc qg, lbt_qdesc qw, const lbt_dgrad_bna* bna, float* dx, void* ws,
                                        int64_t ws_bytes, void* stream) {
  if (!bna || !dx || !desc_ok(d)) return LBT_EINVAL;
  const lbt_dgrad_bna& b = *bna;
  if (!b.R || !b.gb || !b.qn || !b.gout || !b.sums || b.qr.bits <= 0) return LBT_EINVAL;
  if (b.qrg.bits <= 0 || b.qrg.bits > 16 || b.qng.bits <= 0 || b.qng.bits > 16 || d.Cin % 4) return LBT_EINVAL;
  const int64_t rows = (int64_t)d.N * d.H * d.W, inner = (int64_t)d.H * d.W * d.Cin;
  static const int fuse = getenv_int("LBT_DGRAD_BNA", 1);
  IgArgs p;
  if (fuse && dgrad_fused_args(p, gq, wd, ksd, d, qg, qw)) {
    p.has_bna = 1;
    p.perm = igemm_fwdq_perm() >= 2 ? igemm_fwdq_perm() : 1;  // >= 2: the persistent form where it applies
    p.bna = b;
    if (igemm_launch_big(MODE_DGRAD, true, p, (hipStream_t)stream)) return (int)hipGetLastError();
  }
  int rc = lbt_conv_dgrad_igemm_ws(gq, 1, wd, ksd, d, qg, qw, dx, nullptr, ws, ws_bytes, stream);
  if (rc) return rc;
  return lbt_bn_bwd_a_wide_masked(dx, nullptr, nullptr, nullptr, 1, b.qr, b.gb, nullptr, b.qrg, b.R, b.qng, b.qn,
                                  b.gout, nullptr, b.sums, rows, inner, d.Cin, stream);
}

extern "C" int lbt_conv_dgrad_igemm_bn3(const int16_t* gq, const int8_t* wd, int32_t ksd, lbt_conv_desc d,
                                        lbt_qdesc qg, lbt_qdesc qw, const lbt_dgrad_bn3* bn3, float* dx, void* ws,
                                        int64_t ws_bytes, void* stream) {
  if (!bn3 || !dx || !desc_ok(d)) return LBT_EINVAL;
  const lbt_dgrad_bn3& b = *bn3;
  if (!b.g2 || !b.y_bits || b.nbn < 1 || b.nbn > 2 || d.Cin % 4) return LBT_EINVAL;
  for (int k = 0; k < b.nbn; ++k) {
    const lbt_bna_bn& n = b.bn[k];
    if (!n.R || !n.gamma_q || !n.qn || !n.gout || !n.sums) return LBT_EINVAL;
    if (n.qrg.bits <= 0 || n.qrg.bits > 16 || n.qng.bits <= 0 || n.qng.bits > 16) return LBT_EINVAL;
  }
  const int64_t rows = (int64_t)d.N * d.H * d.W, inner = (int64_t)d.H * d.W * d.Cin;
  static const int fuse = getenv_int("LBT_DGRAD_BN3", 1);
  IgArgs p;
  if (fuse && dgrad_fused_args(p, gq, wd, ksd, d, qg, qw)) {
    p.has_bna = 2;
    p.perm = 1;
    p.bn3 = b;
    if (igemm_launch_big(MODE_DGRAD, true, p, (hipStream_t)stream)) return (int)hipGetLastError();
  }
  int rc = lbt_conv_dgrad_igemm_ws(gq, 1, wd, ksd, d, qg, qw, dx, nullptr, ws, ws_bytes, stream);
  for (int k = 0; k < b.nbn && !rc; ++k) {
    const lbt_bna_bn& n = b.bn[k];
    rc = lbt_bn_bwd_a_wide_masked(dx, b.g2, nullptr, b.y_bits, 0, lbt_qdesc{}, n.gamma_q, k == 0 ? b.gmask_out : nullptr,
                                  n.qrg, n.R, n.qng, n.qn, n.gout, nullptr, n.sums, rows, inner, d.Cin, stream);
  }
  return rc;
}
