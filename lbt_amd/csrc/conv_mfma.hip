// conv_mfma.hip -- int8 implicit-GEMM convolution on gfx950 v_mfma_i32_16x16x64_i8.
//
//  lbt_conv_fwd_i8       Conv2d_q.forward  y = conv(Xq, Wq)          (dynamic_fixed_point.py:287-291)
//  lbt_conv_dgrad_i8     Conv2d_q.backward dX = conv^T(gradq, Wq)    (dynamic_fixed_point.py:305)
//  lbt_conv_wgrad_i8     Conv2d_q.backward dW = sum_p Xq (x) gradq   (dynamic_fixed_point.py:302)
//  lbt_conv_wgrad_reduce     + 2*wd*W, dequant, split reduction
//
// Operand maps (probed on MI355X with exact integer data): for 16x16x64_i8 lane l supplies
// A[row l&15][k = 16*(l>>4) .. +15] and B[k = 16*(l>>4) .. +15][col l&15] as 16 int8 each;
// C/D: col = l&15, row = 4*(l>>4) + reg.
//
// fwd / dgrad: GEMM rows = output pixels (fwd) or input pixels (dgrad), cols = output channels,
// k = (tap, 16-channel slice).  Every A fragment is one 16-byte NHWC channel slice of one
// pixel, gathered straight from global memory by its lane (the 9x tap re-reads of a 3x3 conv
// hit L1/L2; the whole activation is a few MB).  B (packed weights, <= 37 KB) is L2-resident.
// Out-of-bounds taps read the encoding of 0: -128 for the unsigned-9-bit offset encoding
// (q - 128), 0 otherwise; the offset is undone in the epilogue with 128 * sum_k W[k][co].
//
// wgrad: GEMM rows = (tap, ci), cols = co, k = pixels.  Each wave stages 64 pixels of G and of
// the tap-shifted X into LDS transposed ([channel][pixel]) and issues 16x16x64 MFMAs; each
// workgroup owns a pixel range and one tap and writes an int32 partial (exact, no atomics).
#include "conv_epilogue.h"
#include "chain_flags.h"
#include "conv_wgrad_body.h"
#include "lds_tr.h"
#include "stem_bwd.h"

#include <algorithm>
#include <utility>

using namespace lbt;

namespace {

constexpr int kThreads = 256;

enum { MODE_FWD = 0, MODE_DGRAD = 1 };

struct GemmArgs {
  const int8_t* a;      // gathered operand (xq for fwd, gq for dgrad), NHWC
  const int8_t* b;      // packed weights [ncol][ks*16]
  int ks;               // 16-byte k-slices per column (multiple of 4)
  int nslices;          // real k-slices = taps * CS
  int a_fill;           // fill word for out-of-bounds taps
  const int32_t* colsum;
  lbt_conv_desc d;
  lbt_qdesc qa, qb;     // scale sources
  float* y;             // fp32 output
  const float* add_src; // fp32 addend (dgrad)
  int8_t* yq;           // quantised output (fwd epilogue quantiser)
  lbt_qdesc qout;
  int64_t* ychsum;
  int64_t M;            // GEMM rows
  int ncol;             // GEMM cols
  lbt_chain_bwd_a chain;  // dgrad epilogue = pass A of this chain (CF != 0)
};

// W4: the B operand (weights) is stored as packed signed 4-bit codes, 8 bytes per 16-element
// k-slice (no int4 MFMA on gfx950 -- unpacked to int8 in registers).
// One workgroup's tile (bid = its index in the GEMM's grid); the body of conv_gemm_kernel and of
// the dgrad half of dgrad_wgrad_kernel.
// DUAL (dgrad with pass A only): p2 is a second dgrad GEMM into the same output pixels (a projection
// block's 1x1/2 shortcut beside its 3x3/2 first conv); its fp32 result float(acc2) * scale2 is the
// pass-A addend, exactly the value the shortcut's own dgrad launch would have stored and this one
// re-loaded as add_src.
template <int MODE, int CS, int NT, int CF, int NB, bool W4, bool DUAL = false>
__device__ __forceinline__ void conv_gemm_body(const GemmArgs& p, uint32_t bid, const GemmArgs* p2 = nullptr) {
  using G = EpiGeom<NT>;
  constexpr int NTW = G::NTW, WPM = G::WPM, MTB = G::MTB;
  __shared__ EpiShared<NT> sh;
  __shared__ ChainShared<NT, (CF ? NB : 1)> csh;
  ChainPre<NT, NB, CF> cp;
  LBT_TS(0);
  const int lane = threadIdx.x & 63, wave = wave_id();
  const int mt_local = wave / WPM;
  const int nt0 = (wave % WPM) * NTW;
  const int64_t mtile = (int64_t)bid * MTB + mt_local;
  const int r = lane & 15, kg = lane >> 4;
  const lbt_conv_desc& d = p.d;
  const bool want_q = p.yq != nullptr;

  // this lane's GEMM row -> pixel (n, y, x) of the "row" space (M < 2^31: 32-bit math)
  const int OH = MODE == MODE_FWD ? d.Ho : d.H, OW = MODE == MODE_FWD ? d.Wo : d.W;
  const int64_t m = mtile * 16 + r;
  const bool row_ok = m < p.M;
  int n = 0, py = 0, px = 0;
  if (row_ok) {
    const uint32_t mu = (uint32_t)m;
    px = (int)(mu % (uint32_t)OW);
    const uint32_t t = mu / (uint32_t)OW;
    py = (int)(t % (uint32_t)OH);
    n = (int)(t / (uint32_t)OH);
  }
  const int cred = CS * 16;  // channels of the gathered operand
  const int SH = MODE == MODE_FWD ? d.H : d.Ho, SW = MODE == MODE_FWD ? d.W : d.Wo;

  // A fragment of k-step kk (slice s = 4*kk + kg) for this lane's row: its address, and the
  // value it takes instead when the slice is padding (0) or the tap is outside the image (fill)
  auto addr_aq = [&](const GemmArgs& q, int kk, bool& use, int& alt) -> const v4i* {
    const lbt_conv_desc& d = q.d;
    const int s = kk * 4 + kg;
    use = false;
    alt = 0;
    if (s >= q.nslices) return reinterpret_cast<const v4i*>(q.a);
    alt = MODE == MODE_DGRAD ? 0 : q.a_fill;
    const int tap = s / CS, cs = s - tap * CS;
    const int kh = tap / d.KW, kw = tap - kh * d.KW;
    int sy, sx;
    bool ok;
    if (MODE == MODE_FWD) {
      sy = py * d.SH + kh - d.PT;
      sx = px * d.SW + kw - d.PL;
      ok = (unsigned)sy < (unsigned)SH && (unsigned)sx < (unsigned)SW;
    } else {
      const int ny = py + d.PT - kh, nx = px + d.PL - kw;
      sy = ny / d.SH;
      sx = nx / d.SW;
      ok = ny >= 0 && nx >= 0 && sy * d.SH == ny && sx * d.SW == nx && sy < SH && sx < SW;
    }
    use = ok && row_ok;
    if (!use) return reinterpret_cast<const v4i*>(q.a);
    return reinterpret_cast<const v4i*>(q.a + (((int64_t)n * SH + sy) * SW + sx) * cred + cs * 16);
  };
  auto addr_a = [&](int kk, bool& use, int& alt) -> const v4i* { return addr_aq(p, kk, use, alt); };
  auto load_bq = [&](const GemmArgs& q, int kk, int j) -> v4i {
    const int col = (nt0 + j) * 16 + r;
    if constexpr (W4)
      return unpack_i4x16(*reinterpret_cast<const v2i*>(q.b + ((int64_t)col * q.ks + kk * 4 + kg) * 8));
    else
      return *reinterpret_cast<const v4i*>(q.b + ((int64_t)col * q.ks + kk * 4 + kg) * 16);
  };
  auto load_b = [&](int kk, int j) -> v4i { return load_bq(p, kk, j); };

  v4i acc[NTW];
#pragma unroll
  for (int j = 0; j < NTW; ++j) acc[j] = v4i{0, 0, 0, 0};
  // epilogue operands, fetched together with the GEMM operands: noise (fwd) / addend (dgrad)
  float ea[NTW][4];
  int corr[NTW];
  const QOut qo{p.yq, p.qout, p.ychsum, p.M, p.ncol, (int64_t)OH * OW};
  const QState qs = qstate(p.qout);

  const int nks = p.ks >> 2;
  // every operand of a 3x3 conv's k loop fits in registers: issue ALL loads (no branches around
  // them), then the MFMAs -- one memory round trip per wave instead of one per k-step
  constexpr int kMaxKS = (9 * CS + 3) / 4;
  const bool preload = nks <= kMaxKS;
  v4i af[kMaxKS], bf[kMaxKS][NTW];
  if (preload) {
    bool use[kMaxKS];
    int alt[kMaxKS];
    const v4i* pa[kMaxKS];
#pragma unroll
    for (int kk = 0; kk < kMaxKS; ++kk) {
      pa[kk] = addr_a(kk < nks ? kk : 0, use[kk], alt[kk]);
      if (kk >= nks) { use[kk] = false; alt[kk] = 0; }  // zero A: its MFMA adds nothing
    }
#pragma unroll
    for (int kk = 0; kk < kMaxKS; ++kk) {
      af[kk] = *pa[kk];
#pragma unroll
      for (int j = 0; j < NTW; ++j) bf[kk][j] = load_b(kk < nks ? kk : 0, j);
    }
    const int* cs_src = (MODE == MODE_FWD && p.colsum) ? p.colsum : zi();
    const uint32_t cmask = (MODE == MODE_FWD && p.colsum) ? 0xffffffffu : 0u;
#pragma unroll
    for (int j = 0; j < NTW; ++j) corr[j] = 128 * cs_src[((nt0 + j) * 16 + r) & cmask];
    if constexpr (CF != 0) {
      chain_prefetch<NT, NB, CF>(p.chain, p.add_src, p.M, p.ncol, (uint32_t)(OH * OW), mtile, nt0, lane, cp);
    } else if constexpr (MODE == MODE_FWD) {
      epi_noise<NTW>(qo, mtile, nt0, lane, ea);
    } else {
      const float* as = p.add_src ? p.add_src : zf();
      const uint32_t amask = p.add_src ? 0xffffffffu : 0u;
#pragma unroll
      for (int j = 0; j < NTW; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int64_t row = mtile * 16 + kg * 4 + i;
          ea[j][i] = as[(uint32_t)((row < p.M ? row : 0) * p.ncol + (nt0 + j) * 16 + r) & amask];
        }
    }
#pragma unroll
    for (int kk = 0; kk < kMaxKS; ++kk)
      if (!use[kk]) af[kk] = v4i{alt[kk], alt[kk], alt[kk], alt[kk]};
#pragma unroll
    for (int kk = 0; kk < kMaxKS; ++kk)
#pragma unroll
      for (int j = 0; j < NTW; ++j) acc[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[kk], bf[kk][j], acc[j], 0, 0, 0);
  } else {
    for (int kk = 0; kk < nks; ++kk) {
      bool use;
      int alt;
      const v4i* pa = addr_a(kk, use, alt);
      v4i a = *pa;
      if (!use) a = v4i{alt, alt, alt, alt};
#pragma unroll
      for (int j = 0; j < NTW; ++j) acc[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, load_b(kk, j), acc[j], 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < NTW; ++j) corr[j] = (MODE == MODE_FWD && p.colsum) ? 128 * p.colsum[(nt0 + j) * 16 + r] : 0;
    if constexpr (CF != 0) {
      chain_prefetch<NT, NB, CF>(p.chain, p.add_src, p.M, p.ncol, (uint32_t)(OH * OW), mtile, nt0, lane, cp);
    } else if constexpr (MODE == MODE_FWD) {
      epi_noise<NTW>(qo, mtile, nt0, lane, ea);
    } else {
#pragma unroll
      for (int j = 0; j < NTW; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int64_t row = mtile * 16 + kg * 4 + i;
          ea[j][i] = (p.add_src && row < p.M) ? p.add_src[row * p.ncol + (nt0 + j) * 16 + r] : 0.f;
        }
    }
  }
  if constexpr (DUAL) {
    static_assert(MODE == MODE_DGRAD && CF != 0, "dual GEMM: dgrad + pass A only");
    const GemmArgs& q = *p2;
    v4i acc2[NTW];
#pragma unroll
    for (int j = 0; j < NTW; ++j) acc2[j] = v4i{0, 0, 0, 0};
    const int nks2 = q.ks >> 2;
    for (int kk = 0; kk < nks2; ++kk) {
      bool use;
      int alt;
      const v4i* pa = addr_aq(q, kk, use, alt);
      v4i a = *pa;
      if (!use) a = v4i{alt, alt, alt, alt};
#pragma unroll
      for (int j = 0; j < NTW; ++j) acc2[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, load_bq(q, kk, j), acc2[j], 0, 0, 0);
    }
    const float scale2 = ldexpf(1.0f, -(frac_exp(q.qa) + frac_exp(q.qb)));
#pragma unroll
    for (int j = 0; j < NTW; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) cp.add[j][i] = (float)acc2[j][i] * scale2;
  }
  LBT_TS(1);

  // ---------------- epilogue: lane owns column (nt0+j)*16 + r of rows mtile*16 + 4*kg + i
  const float scale = ldexpf(1.0f, -(frac_exp(p.qa) + frac_exp(p.qb)));
  float v[NTW][4];
#pragma unroll
  for (int j = 0; j < NTW; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) v[j][i] = (float)(acc[j][i] + corr[j]) * scale;
  if constexpr (CF != 0) {
    LBT_TS(2);
    chain_epi<NT, NB, CF>(p.chain, DUAL || p.add_src != nullptr, p.M, p.ncol, mtile, nt0, wave, lane, v, cp, csh);
    LBT_TS(3);
    return;
  }
  if (!want_q) {
    const bool addv = MODE == MODE_DGRAD && p.add_src;
#pragma unroll
    for (int j = 0; j < NTW; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t row = mtile * 16 + kg * 4 + i;
        if (row < p.M) p.y[row * p.ncol + (nt0 + j) * 16 + r] = addv ? v[j][i] + ea[j][i] : v[j][i];
      }
    return;
  }
  if constexpr (MODE == MODE_FWD) {
    LBT_TS(2);
    epi_quant<NT>(qo, qs, mtile, nt0, wave, lane, v, ea, sh);
    LBT_TS(3);
  }
}

template <int MODE, int CS, int NT, int CF = 0, int NB = 1, bool W4 = false>
__global__ __launch_bounds__(kThreads, (CS == 1 && MODE == MODE_DGRAD && NB == 1) ? 8 : 1) void conv_gemm_kernel(
    GemmArgs p) {
  conv_gemm_body<MODE, CS, NT, CF, NB, W4>(p, blockIdx.x);
}

// dgrad + pass A of a projection block's input gradient: its 3x3/2 conv's dgrad (p) plus the 1x1/2
// shortcut's (p2) in one launch (was: the shortcut's dgrad to an fp32 buffer, then p with it as
// add_src)
template <int CS, int NT, int CF, int NB, bool W4>
__global__ __launch_bounds__(kThreads) void conv_dgrad2_kernel(GemmArgs p, GemmArgs p2) {
  conv_gemm_body<MODE_DGRAD, CS, NT, CF, NB, W4, true>(p, blockIdx.x, &p2);
}

// Two independent GEMMs of one geometry class (same CS / NT / M) in one grid: workgroups [0, nb0)
// run p0's tiles, the rest p1's (a projection block's 3x3/2 conv and its 1x1/2 shortcut, which
// read the same input codes: one launch instead of two).
template <int MODE, int CS, int NT, bool W4>
__global__ __launch_bounds__(kThreads) void conv_gemm2_kernel(GemmArgs p0, GemmArgs p1, uint32_t nb0) {
  if (blockIdx.x < nb0)
    conv_gemm_body<MODE, CS, NT, 0, 1, W4>(p0, blockIdx.x);
  else
    conv_gemm_body<MODE, CS, NT, 0, 1, W4>(p1, blockIdx.x - nb0);
}

template <int CSI>
__global__ __launch_bounds__(kThreads) void conv_wgrad_kernel(WgradArgs wa) {
  __shared__ __attribute__((aligned(16))) WgradShared<CSI> sm;
  conv_wgrad_body<CSI>(wa, blockIdx.x, sm);
}

// Horizontal fusion of one conv's two backward GEMMs, which read the same gradient codes and
// are independent of each other: workgroups [0, nwg) are the wgrad's (the longer ones, dispatched
// first), the rest the dgrad (+ chain pass A) tiles. One launch instead of two; nwg is a multiple
// of 8, so both halves keep their XCD-aware block order.
template <int CS, int NT, int CF, int NB, bool W4>
__global__ __launch_bounds__(kThreads, (CS == 1 && NB == 1) ? 8 : 1) void dgrad_wgrad_kernel(GemmArgs p, WgradArgs wa,
                                                                                          uint32_t nwg) {
  if (blockIdx.x < nwg) {
    __shared__ __attribute__((aligned(16))) WgradShared<NT> sm;
    conv_wgrad_body<NT>(wa, blockIdx.x, sm);
  } else
    conv_gemm_body<MODE_DGRAD, CS, NT, CF, NB, W4>(p, blockIdx.x - nwg);
}

// 256 threads = 32 outputs x 8 split groups; coalesced 128-B slab rows; exact int64 sums.
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const int32_t* __restrict__ slab, int nsplit, int K,
                                                           int Cout, int x_u8off, const int64_t* __restrict__ gcolsum,
                                                           lbt_qdesc qx, lbt_qdesc qg, const float* __restrict__ w,
                                                           float wd2, float* __restrict__ dw,
                                                           long long* __restrict__ num) {
  __shared__ long long red[8][32];
  const int lo = threadIdx.x & 31, sg = threadIdx.x >> 5;
  const int64_t total = (int64_t)K * Cout;
  const int64_t i = (int64_t)blockIdx.x * 32 + lo;
  long long s = 0;
  if (i < total) {
#pragma unroll 4
    for (int b = sg; b < nsplit; b += 8) s += slab[(int64_t)b * total + i];
  }
  red[sg][lo] = s;
  __syncthreads();
  if (sg != 0 || i >= total) return;
  for (int k = 1; k < 8; ++k) s += red[k][lo];
  if (x_u8off && gcolsum) {
    const int co = (int)(i % Cout);
    long long cs = 0;
    for (int k = 0; k < LBT_NSHARD; ++k) cs += gcolsum[(int64_t)k * 2 * Cout + co];
    s += 128ll * cs;
  }
  if (num) {  // the exact exchange: the numerator, dequantised after the all-reduce
    num[i] = s;
    return;
  }
  const float scale = ldexpf(1.0f, -(frac_exp(qx) + frac_exp(qg)));
  const float a = (float)s * scale;
  const float b = wd2 * w[i];
  dw[i] = a + b;
}

template <int MODE, int NT, bool W4>
int launch_gemm_nt(const GemmArgs& p, int cs, hipStream_t st) {
  constexpr int MTB = EpiGeom<NT>::MTB;
  const int64_t mtiles = (p.M + 15) / 16;
  const int64_t blocks = (mtiles + MTB - 1) / MTB;
  if (blocks > 0x7fffffff) return LBT_EINVAL;
  switch (cs) {
    case 1: hipLaunchKernelGGL((conv_gemm_kernel<MODE, 1, NT, 0, 1, W4>), dim3((unsigned)blocks), dim3(kThreads), 0, st, p); break;
    case 2: hipLaunchKernelGGL((conv_gemm_kernel<MODE, 2, NT, 0, 1, W4>), dim3((unsigned)blocks), dim3(kThreads), 0, st, p); break;
    case 4: hipLaunchKernelGGL((conv_gemm_kernel<MODE, 4, NT, 0, 1, W4>), dim3((unsigned)blocks), dim3(kThreads), 0, st, p); break;
    case 8: hipLaunchKernelGGL((conv_gemm_kernel<MODE, 8, NT, 0, 1, W4>), dim3((unsigned)blocks), dim3(kThreads), 0, st, p); break;
    default: return LBT_EINVAL;
  }
  return (int)hipGetLastError();
}

template <int MODE, bool W4 = false>
int launch_gemm(const GemmArgs& p, int cs, hipStream_t st) {
  if (p.M * p.ncol >= (int64_t)1 << 31) return LBT_EINVAL;  // 32-bit row / element arithmetic
  switch (p.ncol / 16) {
    case 1: return launch_gemm_nt<MODE, 1, W4>(p, cs, st);
    case 2: return launch_gemm_nt<MODE, 2, W4>(p, cs, st);
    case 4: return launch_gemm_nt<MODE, 4, W4>(p, cs, st);
    case 8: return launch_gemm_nt<MODE, 8, W4>(p, cs, st);
    default: return LBT_EINVAL;
  }
}


}  // namespace

LBT_TRACE_SETTER(conv)

namespace {
int fwd_setup(const int8_t* xq, int32_t x_u8off, const int8_t* wf, int32_t ksf, const int32_t* wcolsum,
              lbt_conv_desc d, lbt_qdesc qx, lbt_qdesc qw, float* y, int8_t* yq, lbt_qdesc qout, int64_t* ychsum,
              GemmArgs& p) {
  if (!desc_ok(d) || d.Cin % 16 || d.Cout % 16 || d.Cout > 128) return LBT_EINVAL;
  const int cs = d.Cin / 16;
  p.a = xq; p.b = wf; p.ks = ksf; p.nslices = d.KH * d.KW * cs;
  if (ksf % 4 || ksf < p.nslices) return LBT_EINVAL;
  p.a_fill = x_u8off ? (int)0x80808080u : 0;
  p.colsum = x_u8off ? wcolsum : nullptr;
  if (x_u8off && !wcolsum) return LBT_EINVAL;
  if (yq && qout.stochastic && !qout.noise) return LBT_EINVAL;  // quantising epilogue reads the noise table
  if (yq && qout.bits > 8) return LBT_EINVAL;  // int8 codes; the int32 channel sums of q^2 assume |q| <= 2^7
  p.d = d; p.qa = qx; p.qb = qw; p.y = y; p.add_src = nullptr; p.yq = yq; p.qout = qout; p.ychsum = ychsum;
  p.M = (int64_t)d.N * d.Ho * d.Wo; p.ncol = d.Cout;
  return 0;
}

template <bool W4>
int conv_fwd(const int8_t* xq, int32_t x_u8off, const int8_t* wf, int32_t ksf, const int32_t* wcolsum,
             lbt_conv_desc d, lbt_qdesc qx, lbt_qdesc qw, float* y, int8_t* yq, lbt_qdesc qout, int64_t* ychsum,
             void* stream) {
  GemmArgs p;
  const int e = fwd_setup(xq, x_u8off, wf, ksf, wcolsum, d, qx, qw, y, yq, qout, ychsum, p);
  if (e) return e;
  return launch_gemm<MODE_FWD, W4>(p, d.Cin / 16, (hipStream_t)stream);
}

template <int CS, int NT, bool W4>
int launch_fwd_pair(const GemmArgs& p0, const GemmArgs& p1, hipStream_t st) {
  constexpr int MTB = EpiGeom<NT>::MTB;
  const int64_t blocks = ((p0.M + 15) / 16 + MTB - 1) / MTB;
  if (2 * blocks > 0x7fffffff) return LBT_EINVAL;
  hipLaunchKernelGGL((conv_gemm2_kernel<MODE_FWD, CS, NT, W4>), dim3((unsigned)(2 * blocks)), dim3(kThreads), 0, st,
                     p0, p1, (uint32_t)blocks);
  return (int)hipGetLastError();
}

int conv_fwd_pair(const lbt_conv_fwd_job* j0, const lbt_conv_fwd_job* j1, void* stream) {
  if (!j0 || !j1 || j0->w4 != j1->w4) return LBT_EINVAL;
  GemmArgs p[2];
  const lbt_conv_fwd_job* j[2] = {j0, j1};
  for (int i = 0; i < 2; ++i) {
    if (j[i]->w4 && j[i]->qw.bits > 4) return LBT_EINVAL;
    const int e = fwd_setup(j[i]->xq, j[i]->x_u8off, j[i]->wf, j[i]->ksf, j[i]->wcolsum, j[i]->d, j[i]->qx, j[i]->qw,
                            j[i]->y, j[i]->yq, j[i]->qout, j[i]->ychsum, p[i]);
    if (e) return e;
  }
  if (p[0].M != p[1].M || p[0].ncol != p[1].ncol || j0->d.Cin != j1->d.Cin) return LBT_EINVAL;
  if (p[0].M * p[0].ncol >= (int64_t)1 << 31) return LBT_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int key = ((j0->d.Cin / 16) << 8) | ((p[0].ncol / 16) << 1) | (j0->w4 ? 1 : 0);
#define LBT_FP(CS_, NT_)                                                                   \
  if (key == ((CS_ << 8) | (NT_ << 1))) return launch_fwd_pair<CS_, NT_, false>(p[0], p[1], st); \
  if (key == ((CS_ << 8) | (NT_ << 1) | 1)) return launch_fwd_pair<CS_, NT_, true>(p[0], p[1], st);
  // ResNet-20 / CIFAR projection blocks: 16 -> 32 and 32 -> 64 channels
  LBT_FP(1, 2)
  LBT_FP(2, 4)
#undef LBT_FP
  return LBT_EINVAL;
}

template <bool W4>
int conv_dgrad(const int8_t* gq, const int8_t* wd, int32_t ksd, lbt_conv_desc d, lbt_qdesc qg, lbt_qdesc qw,
               float* dx, const float* add_src, void* stream) {
  if (!desc_ok(d) || d.Cin % 16 || d.Cout % 16 || d.Cin > 128) return LBT_EINVAL;
  const int cs = d.Cout / 16;
  GemmArgs p;
  p.a = gq; p.b = wd; p.ks = ksd; p.nslices = d.KH * d.KW * cs;
  if (ksd % 4 || ksd < p.nslices) return LBT_EINVAL;
  p.a_fill = 0; p.colsum = nullptr;
  p.d = d; p.qa = qg; p.qb = qw; p.y = dx; p.add_src = add_src; p.yq = nullptr; p.qout = lbt_qdesc{};
  p.ychsum = nullptr;
  p.M = (int64_t)d.N * d.H * d.W; p.ncol = d.Cin;
  return launch_gemm<MODE_DGRAD, W4>(p, cs, (hipStream_t)stream);
}
}  // namespace

extern "C" int lbt_conv_fwd_i8(const int8_t* xq, int32_t x_u8off, const int8_t* wf, int32_t ksf,
                               const int32_t* wcolsum, lbt_conv_desc d, lbt_qdesc qx, lbt_qdesc qw, float* y,
                               int8_t* yq, lbt_qdesc qout, int64_t* ychsum, void* stream) {
  return conv_fwd<false>(xq, x_u8off, wf, ksf, wcolsum, d, qx, qw, y, yq, qout, ychsum, stream);
}
extern "C" int lbt_conv_fwd_i8w4(const int8_t* xq, int32_t x_u8off, const uint8_t* wf4, int32_t ksf,
                                 const int32_t* wcolsum, lbt_conv_desc d, lbt_qdesc qx, lbt_qdesc qw, float* y,
                                 int8_t* yq, lbt_qdesc qout, int64_t* ychsum, void* stream) {
  if (qw.bits > 4) return LBT_EINVAL;
  return conv_fwd<true>(xq, x_u8off, (const int8_t*)wf4, ksf, wcolsum, d, qx, qw, y, yq, qout, ychsum, stream);
}
extern "C" int lbt_conv_fwd_pair_i8(const lbt_conv_fwd_job* j0, const lbt_conv_fwd_job* j1, void* stream) {
  return conv_fwd_pair(j0, j1, stream);
}
extern "C" int lbt_conv_dgrad_i8(const int8_t* gq, const int8_t* wd, int32_t ksd, lbt_conv_desc d, lbt_qdesc qg,
                                 lbt_qdesc qw, float* dx, const float* add_src, void* stream) {
  return conv_dgrad<false>(gq, wd, ksd, d, qg, qw, dx, add_src, stream);
}
extern "C" int lbt_conv_dgrad_i8w4(const int8_t* gq, const uint8_t* wd4, int32_t ksd, lbt_conv_desc d, lbt_qdesc qg,
                                   lbt_qdesc qw, float* dx, const float* add_src, void* stream) {
  if (qw.bits > 4) return LBT_EINVAL;
  return conv_dgrad<true>(gq, (const int8_t*)wd4, ksd, d, qg, qw, dx, add_src, stream);
}

namespace {

// dgrad + pass A, optionally with the same conv's wgrad in the same launch (wa != nullptr)
template <int CS, int NT, int CF, int NB, bool W4>
int launch_dgrad_chain(const GemmArgs& p, const WgradArgs* wa, uint32_t wblocks, hipStream_t st) {
  constexpr int MTB = EpiGeom<NT>::MTB;
  const int64_t blocks = ((p.M + 15) / 16 + MTB - 1) / MTB;
  if (wa) {
    if (wa->d.Cin != NT * 16 || blocks + wblocks > 0x7fffffff) return LBT_EINVAL;
    hipLaunchKernelGGL((dgrad_wgrad_kernel<CS, NT, CF, NB, W4>), dim3((unsigned)(blocks + wblocks)), dim3(kThreads), 0,
                       st, p, *wa, wblocks);
  } else {
    hipLaunchKernelGGL((conv_gemm_kernel<MODE_DGRAD, CS, NT, CF, NB, W4>), dim3((unsigned)blocks), dim3(kThreads), 0,
                       st, p);
  }
  return (int)hipGetLastError();
}

template <bool W4>
int dgrad_chain(const int8_t* gq, const int8_t* wd, int32_t ksd, lbt_conv_desc d, lbt_qdesc qg, lbt_qdesc qw,
                const float* add_src, const lbt_chain_bwd_a* a, const WgradArgs* wa, uint32_t wblocks, void* stream) {
  if (!desc_ok(d) || d.Cin % 16 || d.Cout % 16 || d.Cin > 128 || !a) return LBT_EINVAL;
  if (a->C != d.Cin || a->rows != d.N || a->inner != (int64_t)d.H * d.W * d.Cin) return LBT_EINVAL;
  const int f = bwd_a_flags(*a);
  if ((f & kAFused) != kAFused) return LBT_EINVAL;
  const lbt_bwd_branch* br[2] = {&a->b1, &a->b2};
  for (int b = 0; b < (a->has_b2 ? 2 : 1); ++b)
    if (!br[b]->qrg.noise || !br[b]->qng.noise || !br[b]->gb) return LBT_EINVAL;
  const int cs = d.Cout / 16;
  GemmArgs p;
  p.a = gq; p.b = wd; p.ks = ksd; p.nslices = d.KH * d.KW * cs;
  if (ksd % 4 || ksd < p.nslices) return LBT_EINVAL;
  p.a_fill = 0; p.colsum = nullptr;
  p.d = d; p.qa = qg; p.qb = qw; p.y = nullptr; p.add_src = add_src; p.yq = nullptr; p.qout = lbt_qdesc{};
  p.ychsum = nullptr;
  p.M = (int64_t)d.N * d.H * d.W; p.ncol = d.Cin;
  p.chain = *a;
  if (p.M * p.ncol >= ((int64_t)1 << 31)) return LBT_EINVAL;  // 32-bit element offsets
  hipStream_t st = (hipStream_t)stream;
  const int nt = d.Cin / 16;
  const int key = (cs << 8) | (nt << 4) | (a->has_b2 ? 1 : 0);
#define LBT_DC(CS_, NT_, CF_, NB_)                                                                  \
  if (key == ((CS_ << 8) | (NT_ << 4) | (NB_ == 2)) && f == (CF_))                                  \
    return launch_dgrad_chain<CS_, NT_, CF_, NB_, W4>(p, wa, wblocks, st);
#define LBT_DC_SHAPES(CF_, NB_) \
  LBT_DC(1, 1, CF_, NB_) LBT_DC(2, 2, CF_, NB_) LBT_DC(4, 4, CF_, NB_) LBT_DC(2, 1, CF_, NB_) LBT_DC(4, 2, CF_, NB_)
  LBT_DC_SHAPES(kAFused | kAMaskR, 1)             // block, first BN (mask from R1)
  LBT_DC_SHAPES(kAFused | kAYMask | kAGmask, 1)   // block end, identity shortcut
  LBT_DC_SHAPES(kAFused | kAYMask, 2)             // block end, projection shortcut
  LBT_DC_SHAPES(kAFused | kAYMask, 1)             // stem
#undef LBT_DC_SHAPES
#undef LBT_DC
  return LBT_EINVAL;
}

template <int CS, int NT, int CF, int NB, bool W4>
int launch_dgrad2(const GemmArgs& p, const GemmArgs& p2, hipStream_t st) {
  constexpr int MTB = EpiGeom<NT>::MTB;
  const int64_t blocks = ((p.M + 15) / 16 + MTB - 1) / MTB;
  hipLaunchKernelGGL((conv_dgrad2_kernel<CS, NT, CF, NB, W4>), dim3((unsigned)blocks), dim3(kThreads), 0, st, p, p2);
  return (int)hipGetLastError();
}

// dgrad (gq, wd, d) + dgrad (gq2, wd2, d2) + pass A, one launch (see conv_dgrad2_kernel)
template <bool W4>
int dgrad2_chain(const int8_t* gq, const int8_t* wd, int32_t ksd, lbt_conv_desc d, lbt_qdesc qg, lbt_qdesc qw,
                 const int8_t* gq2, const int8_t* wd2, int32_t ksd2, lbt_conv_desc d2, lbt_qdesc qg2, lbt_qdesc qw2,
                 const lbt_chain_bwd_a* a, void* stream) {
  if (!desc_ok(d) || !desc_ok(d2) || d.Cin % 16 || d.Cout % 16 || d.Cin > 128 || !a) return LBT_EINVAL;
  // same input-gradient pixels and channels, same gathered-gradient geometry
  if (d2.N != d.N || d2.H != d.H || d2.W != d.W || d2.Cin != d.Cin || d2.Cout != d.Cout || d2.Ho != d.Ho ||
      d2.Wo != d.Wo)
    return LBT_EINVAL;
  if (a->C != d.Cin || a->rows != d.N || a->inner != (int64_t)d.H * d.W * d.Cin) return LBT_EINVAL;
  const int f = bwd_a_flags(*a);
  if ((f & kAFused) != kAFused) return LBT_EINVAL;
  const lbt_bwd_branch* br[2] = {&a->b1, &a->b2};
  for (int b = 0; b < (a->has_b2 ? 2 : 1); ++b)
    if (!br[b]->qrg.noise || !br[b]->qng.noise || !br[b]->gb) return LBT_EINVAL;
  const int cs = d.Cout / 16;
  GemmArgs p, p2;
  p.a = gq; p.b = wd; p.ks = ksd; p.nslices = d.KH * d.KW * cs;
  p2.a = gq2; p2.b = wd2; p2.ks = ksd2; p2.nslices = d2.KH * d2.KW * cs;
  if (ksd % 4 || ksd < p.nslices || ksd2 % 4 || ksd2 < p2.nslices) return LBT_EINVAL;
  p.a_fill = p2.a_fill = 0; p.colsum = p2.colsum = nullptr;
  p.d = d; p.qa = qg; p.qb = qw; p.y = nullptr; p.add_src = nullptr; p.yq = nullptr; p.qout = lbt_qdesc{};
  p.ychsum = nullptr;
  p.M = (int64_t)d.N * d.H * d.W; p.ncol = d.Cin;
  p.chain = *a;
  p2.d = d2; p2.qa = qg2; p2.qb = qw2; p2.y = nullptr; p2.add_src = nullptr; p2.yq = nullptr; p2.qout = lbt_qdesc{};
  p2.ychsum = nullptr; p2.M = p.M; p2.ncol = p.ncol; p2.chain = lbt_chain_bwd_a{};
  if (p.M * p.ncol >= ((int64_t)1 << 31)) return LBT_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int nt = d.Cin / 16;
  const int key = (cs << 8) | (nt << 4) | (a->has_b2 ? 1 : 0);
#define LBT_D2(CS_, NT_, CF_, NB_)                                                                \
  if (key == ((CS_ << 8) | (NT_ << 4) | (NB_ == 2)) && f == (CF_))                                  \
    return launch_dgrad2<CS_, NT_, CF_, NB_, W4>(p, p2, st);
  // projection blocks (Cout = 2 Cin) whose input gradient feeds an identity block's end chain or
  // the stem's
  LBT_D2(2, 1, kAFused | kAYMask | kAGmask, 1) LBT_D2(4, 2, kAFused | kAYMask | kAGmask, 1)
  LBT_D2(2, 1, kAFused | kAYMask, 1) LBT_D2(4, 2, kAFused | kAYMask, 1)
#undef LBT_D2
  return LBT_EINVAL;
}

template <bool W4>
int dgrad_chain_wgrad(const int8_t* gq, const int8_t* wd, int32_t ksd, lbt_conv_desc d, lbt_qdesc qg, lbt_qdesc qw,
                      const float* add_src, const lbt_chain_bwd_a* a, const int8_t* xq, int32_t x_u8off,
                      int32_t* slab, int32_t nsplit, int32_t nshard, void* stream) {
  WgradArgs wa;
  uint32_t wblocks = 0;
  const int e = wgrad_setup(xq, x_u8off, gq, d, slab, nsplit, nshard, wa, wblocks);
  if (e) return e;
  return dgrad_chain<W4>(gq, wd, ksd, d, qg, qw, add_src, a, &wa, wblocks, stream);
}

}  // namespace

extern "C" int lbt_conv_dgrad2_chain_i8(const int8_t* gq, const int8_t* wd, int32_t ksd, lbt_conv_desc d, lbt_qdesc qg,
                                        lbt_qdesc qw, const int8_t* gq2, const int8_t* wd2, int32_t ksd2,
                                        lbt_conv_desc d2, lbt_qdesc qg2, lbt_qdesc qw2, int32_t w4,
                                        const lbt_chain_bwd_a* a, void* stream) {
  if (w4) {
    if (qw.bits > 4 || qw2.bits > 4) return LBT_EINVAL;
    return dgrad2_chain<true>(gq, wd, ksd, d, qg, qw, gq2, wd2, ksd2, d2, qg2, qw2, a, stream);
  }
  return dgrad2_chain<false>(gq, wd, ksd, d, qg, qw, gq2, wd2, ksd2, d2, qg2, qw2, a, stream);
}
extern "C" int lbt_conv_dgrad_chain_i8(const int8_t* gq, const int8_t* wd, int32_t ksd, lbt_conv_desc d, lbt_qdesc qg,
                                       lbt_qdesc qw, const float* add_src, const lbt_chain_bwd_a* a, void* stream) {
  return dgrad_chain<false>(gq, wd, ksd, d, qg, qw, add_src, a, nullptr, 0, stream);
}
extern "C" int lbt_conv_dgrad_chain_i8w4(const int8_t* gq, const uint8_t* wd4, int32_t ksd, lbt_conv_desc d,
                                         lbt_qdesc qg, lbt_qdesc qw, const float* add_src, const lbt_chain_bwd_a* a,
                                         void* stream) {
  if (qw.bits > 4) return LBT_EINVAL;
  return dgrad_chain<true>(gq, (const int8_t*)wd4, ksd, d, qg, qw, add_src, a, nullptr, 0, stream);
}
extern "C" int lbt_conv_dgrad_chain_wgrad_i8(const int8_t* gq, const int8_t* wd, int32_t ksd, lbt_conv_desc d,
                                             lbt_qdesc qg, lbt_qdesc qw, const float* add_src,
                                             const lbt_chain_bwd_a* a, const int8_t* xq, int32_t x_u8off,
                                             int32_t* slab, int32_t nsplit, int32_t nshard, void* stream) {
  return dgrad_chain_wgrad<false>(gq, wd, ksd, d, qg, qw, add_src, a, xq, x_u8off, slab, nsplit, nshard, stream);
}
extern "C" int lbt_conv_dgrad_chain_wgrad_i8w4(const int8_t* gq, const uint8_t* wd4, int32_t ksd, lbt_conv_desc d,
                                               lbt_qdesc qg, lbt_qdesc qw, const float* add_src,
                                               const lbt_chain_bwd_a* a, const int8_t* xq, int32_t x_u8off,
                                               int32_t* slab, int32_t nsplit, int32_t nshard, void* stream) {
  if (qw.bits > 4) return LBT_EINVAL;
  return dgrad_chain_wgrad<true>(gq, (const int8_t*)wd4, ksd, d, qg, qw, add_src, a, xq, x_u8off, slab, nsplit,
                                 nshard, stream);
}

extern "C" int lbt_conv_wgrad_i8(const int8_t* xq, int32_t x_u8off, const int8_t* gq, lbt_conv_desc d,
                                    int32_t* slab, int32_t nsplit, int32_t nshard, void* stream) {
  WgradArgs wa;
  uint32_t blocks = 0;
  const int e = wgrad_setup(xq, x_u8off, gq, d, slab, nsplit, nshard, wa, blocks);
  if (e) return e;
  hipStream_t st = (hipStream_t)stream;
  switch (d.Cin / 16) {
    case 1: hipLaunchKernelGGL(conv_wgrad_kernel<1>, dim3(blocks), dim3(kThreads), 0, st, wa); break;
    case 2: hipLaunchKernelGGL(conv_wgrad_kernel<2>, dim3(blocks), dim3(kThreads), 0, st, wa); break;
    case 4: hipLaunchKernelGGL(conv_wgrad_kernel<4>, dim3(blocks), dim3(kThreads), 0, st, wa); break;
    case 8: hipLaunchKernelGGL(conv_wgrad_kernel<8>, dim3(blocks), dim3(kThreads), 0, st, wa); break;
    default: return LBT_EINVAL;
  }
  return (int)hipGetLastError();
}

// ---- many convs' weight gradients in ONE launch (lbt_conv_wgrad_many_i8): the jobs travel in the
// kernel arguments; job j owns blocks [start[j], start[j+1]) (multiples of 8: each job keeps its
// XCD-aware unit order). 3x3 / stride-1 / SAME jobs whose image rows tile 64-pixel chunks run
// wgrad_s1_body, the others conv_wgrad_body (one unit = pixel split x tap x co slice).
//
// wgrad_s1_body<NCO, NH>: workgroup = (pixel split, ci slice, group of NCO co slices) of kFW waves. A
// wave takes 64 consecutive output pixels at a time (whole image rows: 64 % W == 0, H % (64 / W) == 0)
// and stages, by LDS-DMA into its own ring of kWgmBufs buffers, the X slices of those rows plus a
// one-pixel halo ([64/W + 2][W + 2][16 B] in NH pieces of 64 slices, the fill code outside the image)
// and the pixels' NCO * 16 contiguous G bytes; all 9 * NCO MFMAs run from that image with per-lane
// transposed reads. X leaves L2 once per (ci slice, co group) and G once per ci slice instead of once
// per (ci, co) slice pair, and the LDS image and the wave-uniform chunk arithmetic are paid once for
// 9 * NCO MFMAs. The staging holds no registers, which is what leaves room for the 36 * NCO accumulator
// registers at two workgroups per CU. The waves' partials are summed in LDS, one co slice at a time,
// and added into the job's slab (shard = split % nshard) with one integer atomic per output.
// Exactness: an int32 accumulator of a wave sums at most 65536 pixels and a slab shard covers at most
// 65536 pixels (|x * g| <= 255 * 128 < 2^15); both are checked on the host (wgrad_setup,
// wgrad_s1_variant). The sums are integers, so any split and any order give the same slab totals.
namespace {
constexpr int kMaxWJobs = 24;
constexpr int kWgmOcc = 4;    // waves per SIMD the batched launch's registers are budgeted for: 2 workgroups per CU
constexpr int kWgmBufs = 2;   // chunks in flight per wave (LDS-DMA ring)
constexpr int kWgmBuf = 4096; // bytes of one ring buffer: NH KB of X halo slices | NCO KB of G
constexpr int kFW = 8;        // waves per workgroup of the batched launch
// The plan's defaults (lbt_conv_wgrad_many_nsplit): at 128 images the ResNet-20 launch, the stem's 256
// workgroups included, then has fewer workgroups than are resident at once (2 per CU), so none waits for
// another to end; a workgroup costs about 10 us whatever its share of the work
constexpr int kWgmCpw = 16;        // default 64-pixel chunks per wave of a staged job
constexpr int kWgmMinUnits = 8;    // workgroups per staged job, at least (while a wave keeps one chunk)
constexpr int kWgmTapUnits = 16;   // workgroups per per-tap job, about
constexpr int kHaloMax = 3;   // halo pieces per chunk of the stride-1 instances: (64/W + 2) * (W + 2) <= 192
struct WgradMany {
  WgradArgs j[kMaxWJobs];
  uint32_t start[kMaxWJobs + 1];
  int32_t fast[kMaxWJobs];  // 0: conv_wgrad_body; else wgrad_s1_variant
  int n;
};
union WgradManyShared {
  WgradShared<1, kFW> s1;
  WgradShared<2, kFW> s2;
  int8_t stage[kFW][kWgmBufs * kWgmBuf];     // wgrad_s1_body: per wave the ring of X halo | G images
  // wgrad_s1_body: partials [tap][kg][r][4] of wave pair (w, w + kFW/2), summed in place, one co slice
  // at a time (both slices at once need 72 KB: measured 2.7 us slower, the launch no longer keeps two
  // workgroups per CU)
  int red[kFW / 2][9 * 256];
};

// The staged body's instance for this conv and split: 0 none (conv_wgrad_body takes it), else
// 1 <NCO 1, NH 3>, 2 <NCO 1, NH 2>, 3 <NCO 2, NH 2> (3x3 / 1 SAME; one ring buffer holds NH + NCO <= 4 KB),
// 4 <NCO 2, NH 5, stride 2, one buffer> (3x3 / 2)
int wgrad_s1_variant(const lbt_conv_desc& d, int nsplit) {
  if (d.KH != 3 || d.KW != 3 || d.SH != d.SW || (d.SH != 1 && d.SH != 2) || d.PT < 0 || d.PT > 1 || d.PL < 0 ||
      d.PL > 1 || d.Wo <= 0 || d.Wo > 64 || 64 % d.Wo || d.Ho % (64 / d.Wo))
    return 0;
  if (d.SH == 1 && (d.PT != 1 || d.PB != 1 || d.PL != 1 || d.PR != 1 || d.Ho != d.H || d.Wo != d.W)) return 0;
  const int64_t chunks = (int64_t)d.N * d.Ho * d.Wo / 64;
  if (nsplit <= 0 || chunks % nsplit) return 0;
  // a wave walks ceil(chunks per split / kFW) chunks of 64 pixels: at most 65536 pixels per accumulator
  if ((chunks / nsplit + kFW - 1) / kFW * 64 > 65536) return 0;
  const int nhalo = ((64 / d.Wo - 1) * d.SH + 3) * ((d.Wo - 1) * d.SH + 3), nh = (nhalo + 63) / 64;
  const bool co2 = (d.Cout / 16) % 2 == 0;
  if (d.SH == 2) return (co2 && nh <= 5) ? 4 : 0;
  if (nh > kHaloMax) return 0;
  if (nh == 3) return 1;
  return co2 ? 3 : 2;
}
int wgrad_s1_nco(int variant) { return variant >= 3 ? 2 : 1; }

static __device__ __attribute__((aligned(16))) uint32_t kWgFill80[4] = {0x80808080u, 0x80808080u, 0x80808080u,
                                                                        0x80808080u};
typedef __attribute__((address_space(3))) void* wg_lds_vptr;
template <int N>
LBT_DEV void wg_vm_wait() {
  static_assert(N >= 0 && N < 64, "vmcnt");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// ds_read_b64_tr_b8 as inline asm: the compiler's waitcnt pass makes every ds_read_tr intrinsic wait
// for ALL outstanding LDS-DMA (vmcnt(0): it cannot tell the ring's buffers apart), which would
// serialise the ring. The asm form is invisible to it, so its results are fenced by hand (wg_tr_wait:
// s_waitcnt lgkmcnt(0) taking the fragments as in/out operands, so no use moves above it).
template <int OFF>
LBT_DEV v4i wg_tr_frag(uint32_t a, uint32_t b) {
  v2i lo, hi;
  asm volatile("ds_read_b64_tr_b8 %0, %1 offset:%2" : "=v"(lo) : "v"(a), "n"(OFF) : "memory");
  asm volatile("ds_read_b64_tr_b8 %0, %1 offset:%2" : "=v"(hi) : "v"(b), "n"(OFF) : "memory");
  return v4i{lo.x, lo.y, hi.x, hi.y};
}
LBT_DEV void wg_tr_wait(v4i& a) { asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a)::"memory"); }
LBT_DEV void wg_tr_wait(v4i& a, v4i& b) { asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b)::"memory"); }
LBT_DEV void wg_tr_wait(v4i& a, v4i& b, v4i& c) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b), "+v"(c)::"memory");
}

template <int I>
using wg_int = std::integral_constant<int, I>;
template <class F, int... I>
LBT_DEV void wg_static_for(F&& f, std::integer_sequence<int, I...>) {
  (f(wg_int<I>{}), ...);
}

template <int NCO, int NH, int S = 1, int NB = kWgmBufs>
__device__ __forceinline__ void wgrad_s1_body(const WgradArgs& wa, uint32_t bid, WgradManyShared& sm) {
  constexpr int kBuf = kWgmBufs * kWgmBuf / NB;  // bytes of one of this instance's NB buffers
  static_assert((NH + NCO) * 1024 <= kBuf && (NB == 1 || NB == kWgmBufs), "one ring buffer");
  const lbt_conv_desc& d = wa.d;
  const int H = d.H, W = d.W, Wo = d.Wo, Cin = d.Cin, Cout = d.Cout;
  const int ncs = Cin >> 4, ncog = (Cout >> 4) / NCO, nsplit = wa.nsplit;
  const int total = nsplit * ncs * ncog;
  const int xchunk = (total + 7) >> 3;
  const int u = (int)(bid & 7) * xchunk + (int)(bid >> 3);  // XCD-aware: a split's slices share an L2
  if (u >= total) return;
  const int split = u / (ncs * ncog), urem = u - split * (ncs * ncog);
  const int cis = urem / ncog, cog = urem - cis * ncog;
  const int lane = threadIdx.x & 63, wave = wave_id();
  const int j = lane & 15, kg = lane >> 4;
  // a chunk = RB whole output rows; its input window = WR rows x Wp columns from input pixel
  // (S * first output row - PT, -PL)
  const int RB = 64 / Wo, WR = (RB - 1) * S + 3, Wp = (Wo - 1) * S + 3, nhalo = WR * Wp;
  const int bpi = d.Ho / RB;                                // chunks (row blocks) per image
  const int cps = (int)((int64_t)d.N * bpi / nsplit);       // chunks per split (exact: host check)
  const int c0 = split * cps;
  const int nmine = cps > wave ? (cps - wave + kFW - 1) / kFW : 0;
  const int8_t* xfill = wa.x_fill ? reinterpret_cast<const int8_t*>(kWgFill80) : reinterpret_cast<const int8_t*>(zi());
  const int8_t* zero = reinterpret_cast<const int8_t*>(zi());
  int8_t* region = sm.stage[wave];
  typedef __attribute__((address_space(3))) int8_t wg_lds_i8;
  const uint32_t rbase = (uint32_t)(uintptr_t)(wg_lds_i8*)region;  // LDS byte address of this wave's ring
  // per-lane transposed-read addresses in ring buffer 0 (chunk-invariant): pixels pa = 16kg + j/2 and
  // pa + 8; X by kernel row (the tap's column and the ring buffer are immediate offsets), G slice 0
  const int pa = 16 * kg + (j >> 1), pb = pa + 8;
  uint32_t xa[3], xb[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    xa[r] = rbase + (uint32_t)((((pa / Wo) * S + r) * Wp + (pa % Wo) * S) * 16 + 8 * (j & 1));
    xb[r] = rbase + (uint32_t)((((pb / Wo) * S + r) * Wp + (pb % Wo) * S) * 16 + 8 * (j & 1));
  }
  const uint32_t ga = rbase + (uint32_t)(NH * 1024 + pa * 16 * NCO + 8 * (j & 1));
  const uint32_t gb = rbase + (uint32_t)(NH * 1024 + pb * 16 * NCO + 8 * (j & 1));
  // chunk-invariant geometry of this lane's halo slices t = lane + 64 i of the [WR][Wp] window: the
  // offset from input pixel (S * first output row, 0), whether it is a real column inside the window,
  // whether it lies in a window row above the image at the first row block / below it at the last; and of
  // its G pieces q = lane + 64 c of the chunk's [64 px][NCO][16 B] block. The per-chunk part is wave-uniform.
  const int hbot0 = H - (d.Ho - RB) * S + d.PT;  // window rows >= this are below the image at the last row block
  int hoff[NH], goff[NCO];
  uint32_t hin = 0, htop = 0, hbot = 0;
#pragma unroll
  for (int i = 0; i < NH; ++i) {
    const int t = lane + 64 * i;
    const int hy = t / Wp, hx = t - hy * Wp;
    hoff[i] = ((hy - d.PT) * W + hx - d.PL) * Cin;
    hin |= (uint32_t)(t < nhalo && hx >= d.PL && hx < W + d.PL) << i;
    htop |= (uint32_t)(hy < d.PT) << i;
    hbot |= (uint32_t)(hy >= hbot0) << i;
  }
#pragma unroll
  for (int c = 0; c < NCO; ++c) {
    const int q = lane + 64 * c;
    goff[c] = (q / NCO) * Cout + (cog * NCO + q % NCO) * 16;
  }
  v4i acc[9][NCO];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int c = 0; c < NCO; ++c) acc[t][c] = v4i{0, 0, 0, 0};

  // The wave's chunks are c0 + wave + kFW s, s < nmine; issue() is called for s = 0, 1, 2, ... in order
  // and carries the chunk, its image and its row block within the image along (no division per chunk).
  // A step past the end re-stages the last chunk's X with zero G: every DMA is unconditional, so the
  // counted vmcnt waits below are exact.
  constexpr int kDma = NH + NCO;  // DMA instructions per chunk
  int ic = c0 + wave, in = ic / bpi, im = ic - in * bpi;
  const int instep = kFW / bpi, imstep = kFW - instep * bpi;
  auto issue = [&](int k, int s) {
    // wave-uniform: the chunk's first output pixel and its window's origin row, RB whole rows of image in
    const int64_t p0 = (int64_t)ic * 64, x0 = ((int64_t)in * H + im * (RB * S)) * W;
    const int8_t* xim = wa.xq + (x0 * Cin + cis * 16);
    const uint32_t valid = hin & ~(im == 0 ? htop : 0u) & ~(im == bpi - 1 ? hbot : 0u);
    int8_t* b = region + k * kBuf;
#pragma unroll
    for (int i = 0; i < NH; ++i)
      __builtin_amdgcn_global_load_lds((valid >> i) & 1 ? xim + hoff[i] : xfill, (wg_lds_vptr)(b + i * 1024), 16, 0, 0);
    const int8_t* gim = wa.gq + p0 * Cout;
#pragma unroll
    for (int c = 0; c < NCO; ++c)
      __builtin_amdgcn_global_load_lds(s < nmine ? gim + goff[c] : zero, (wg_lds_vptr)(b + (NH + c) * 1024), 16, 0, 0);
    if (s + 1 < nmine) {
      ic += kFW;
      in += instep;
      im += imstep;
      if (im >= bpi) {
        im -= bpi;
        ++in;
      }
    }
  };
  LBT_TS(0);
  if (nmine > 0) {  // NB == 1: one chunk at a time (the strided instance's window takes the whole region)
    if constexpr (NB > 1) {
#pragma unroll
      for (int k = 0; k < NB; ++k) issue(k, k);
    }
    for (int s = 0; s < nmine; s += NB) {
      wg_static_for(
          [&](auto K) {
            constexpr int k = decltype(K)::value, kb = k * kBuf;
            if constexpr (NB == 1) issue(0, s);
            wg_vm_wait<(NB - 1) * kDma>();  // chunk s + k landed; the younger chunk may be in flight
            v4i bf[NCO];
            wg_static_for([&](auto C) { bf[decltype(C)::value] = wg_tr_frag<kb + decltype(C)::value * 16>(ga, gb); },
                          std::make_integer_sequence<int, NCO>{});
            v4i af = wg_tr_frag<kb>(xa[0], xb[0]);
            if constexpr (NCO == 2)
              wg_tr_wait(bf[0], bf[1], af);
            else
              wg_tr_wait(bf[0], af);
            wg_static_for(
                [&](auto T) {  // tap t + 1's fragment is read under tap t's MFMAs
                  constexpr int t = decltype(T)::value;
                  v4i an = af;
                  if constexpr (t < 8) an = wg_tr_frag<kb + ((t + 1) % 3) * 16>(xa[(t + 1) / 3], xb[(t + 1) / 3]);
#pragma unroll
                  for (int c = 0; c < NCO; ++c)
                    acc[t][c] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af, bf[c], acc[t][c], 0, 0, 0);
                  if constexpr (t < 8) {
                    wg_tr_wait(an);
                    af = an;
                  }
                },
                std::make_integer_sequence<int, 9>{});
            if constexpr (NB > 1) issue(k, s + k + NB);  // this buffer's reads are done (the last wg_tr_wait)
          },
          std::make_integer_sequence<int, NB>{});
    }
    wg_vm_wait<0>();  // the trailing (clamped) DMAs: nothing may still write LDS past here
  }
  LBT_TS(1);
  // acc[t][c] element i: ci = 4kg + i, co = j of co slice cog * NCO + c (16x16 C/D map); waves w and
  // w + kFW/2 share slot w; one co slice at a time
  constexpr int kHalf = kFW / 2;
#pragma unroll
  for (int c = 0; c < NCO; ++c) {
    __syncthreads();  // the partials overwrite the staging regions / the previous slice's partials
    if (wave < kHalf) {
#pragma unroll
      for (int t = 0; t < 9; ++t) *reinterpret_cast<v4i*>(&sm.red[wave][(t * 64 + lane) * 4]) = acc[t][c];
    }
    __syncthreads();
    if (wave >= kHalf) {
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        v4i* q = reinterpret_cast<v4i*>(&sm.red[wave - kHalf][(t * 64 + lane) * 4]);
        *q = *q + acc[t][c];
      }
    }
    __syncthreads();
    if (c == 0) LBT_TS(2);
    int32_t* dst = wa.slab + (int64_t)(split % wa.nshard) * 9 * Cin * Cout + (int64_t)cis * 16 * Cout +
                   (cog * NCO + c) * 16;
    for (int i = threadIdx.x; i < 9 * 256; i += kFW * 64) {
      int v = 0;
#pragma unroll
      for (int w = 0; w < kHalf; ++w) v += sm.red[w][i];
      const int t = i >> 8, l = (i >> 2) & 63, ii = i & 3;
      const int ci = 4 * (l >> 4) + ii, co = l & 15;
      if (v) LBT_GADD(&dst[((int64_t)t * Cin + ci) * Cout + co], v);  // integer atomics: exact, order-independent
    }
  }
  LBT_TS(3);
}

// block b of a batched launch: find its job, run that job's body
LBT_DEV void wgrad_many_block(const WgradMany& m, uint32_t b, WgradManyShared& sm) {
  int j = 0;
#pragma unroll 1
  while (j + 1 < m.n && b >= m.start[j + 1]) ++j;
  const WgradArgs& wa = m.j[j];
  const uint32_t rb = b - m.start[j];
#ifdef LBT_TRACE
  if (threadIdx.x == 0 && lbt_trace_buf) lbt_trace_buf[(size_t)blockIdx.x * 8 + 6] = (unsigned long long)(j + 1);
#endif
  switch (m.fast[j]) {  // wgrad_s1_variant
    case 1: wgrad_s1_body<1, 3>(wa, rb, sm); return;
    case 2: wgrad_s1_body<1, 2>(wa, rb, sm); return;
    case 3: wgrad_s1_body<2, 2>(wa, rb, sm); return;
    case 4: wgrad_s1_body<2, 5, 2, 1>(wa, rb, sm); return;
    default: break;
  }
  switch (wa.d.Cin >> 4) {
    case 1: conv_wgrad_body<1, kFW>(wa, rb, sm.s1); break;
    default: conv_wgrad_body<2, kFW>(wa, rb, sm.s2); break;
  }
}

__global__ __launch_bounds__(kFW * 64, kWgmOcc) void conv_wgrad_many_kernel(const WgradMany m) {
  __shared__ __attribute__((aligned(16))) WgradManyShared sm;
  wgrad_many_block(m, blockIdx.x, sm);
}

// The batched weight gradients with the stem's whole backward (stem_bwd.h, two 256-pixel row blocks
// per 512-thread workgroup) as extra blocks of the same launch: the stem backward reads only the first
// block's dgrad output, like the batched jobs, so it shares the batched launch's rounds of workgroups
// instead of running as a launch of its own after it (lbt_conv_wgrad_many_stem_i8; 25.2 + 13.0 us as
// two launches -> 34.2 us as one).
union WgradManyStemShared {
  WgradManyShared w;
  StemBwdShared<2> s;
};
static_assert(kFW * 64 == 2 * 256, "two stem row blocks per workgroup of the batched launch");
// (stem_first, the default: the stem's workgroups are the launch's FIRST blocks; else its last)
__global__ __launch_bounds__(kFW * 64, kWgmOcc) void conv_wgrad_many_stem_kernel(const WgradMany m,
                                                                                    const StemBwdArgs st,
                                                                                    uint32_t pairs, int stem_first) {
  __shared__ __attribute__((aligned(16))) WgradManyStemShared sm;
  const uint32_t b = blockIdx.x, nw = m.start[m.n];
  if (stem_first ? b < pairs : b >= nw) {
    stem_bwd_body<2>(st, stem_first ? b : b - nw, sm.s);
    return;
  }
  wgrad_many_block(m, stem_first ? b - pairs : b, sm.w);
}
static_assert(sizeof(WgradMany) + sizeof(StemBwdArgs) + 8 <= 4096, "kernel arguments");
static_assert(sizeof(WgradMany) <= 4096, "kernel arguments");

// WgradArgs + block count of one job of the batched launch
int wgrad_many_setup(const lbt_wgrad_job& w, WgradArgs& wa, uint32_t& blocks, int32_t& fast) {
  if (!w.slab || !w.xq || !w.gq) return LBT_EINVAL;
  const int e = wgrad_setup(w.xq, w.x_u8off, w.gq, w.d, w.slab, w.nsplit, w.nshard, wa, blocks);
  if (e) return e;
  fast = wgrad_s1_variant(w.d, w.nsplit);
  if (fast) {
    const int64_t units = (int64_t)w.nsplit * (w.d.Cin / 16) * (w.d.Cout / 16 / wgrad_s1_nco(fast));
    blocks = (uint32_t)((units + 7) / 8 * 8);
  } else if (w.d.Cin != 16 && w.d.Cin != 32) {
    return LBT_EINVAL;  // conv_wgrad_body<CSI, kFW> instances: CSI 1, 2
  }
  return 0;
}
}  // namespace

// ---- the batched launch's plan: one host-only definition for the library and the Python planner.
// Resident workgroups of the batched launch: CUs x the kFW-wave workgroups that kWgmOcc waves per
// SIMD admit (the kernels' launch bounds; registers and LDS both allow exactly that: tools/kres.py).
extern "C" int lbt_conv_wgrad_many_slots(void) {
  static const int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;  // MI355X
    return n;
  }();
  return cus * (kWgmOcc * 4 / kFW);
}

// Workgroups of conv d's job at nsplit pixel splits (a multiple of 8), -LBT_EINVAL for a job the launch
// does not take.
extern "C" int lbt_conv_wgrad_many_blocks(lbt_conv_desc d, int32_t nsplit) {
  if (!desc_ok(d) || d.Cin % 16 || d.Cout % 16 || nsplit <= 0) return -LBT_EINVAL;
  const int v = wgrad_s1_variant(d, nsplit);
  if (!v && d.Cin != 16 && d.Cin != 32) return -LBT_EINVAL;
  const int64_t units = v ? (int64_t)nsplit * (d.Cin / 16) * (d.Cout / 16 / wgrad_s1_nco(v))
                          : (int64_t)nsplit * d.KH * d.KW * (d.Cout / 16);
  return units < ((int64_t)1 << 30) ? (int)((units + 7) / 8 * 8) : -LBT_EINVAL;
}

// Pixel splits of conv d's job. Staged instances (wgrad_s1_variant): a split is kFW waves x
// chunks_per_wave 64-pixel chunks, rounded down to a divisor of the chunk count; per-tap jobs:
// about tap_units workgroups (split x tap x co slice) of at least 512 pixels. 0 selects the default
// of either argument.
extern "C" int lbt_conv_wgrad_many_nsplit(lbt_conv_desc d, int32_t chunks_per_wave, int32_t tap_units) {
  if (!desc_ok(d) || d.Cin % 16 || d.Cout % 16) return -LBT_EINVAL;
  const int64_t P = (int64_t)d.N * d.Ho * d.Wo;
  const int v = wgrad_s1_variant(d, 1);
  if (!v) {
    const int64_t lo = (P + 65535) / 65536, taps = (int64_t)d.KH * d.KW * (d.Cout / 16);
    const int64_t want = std::max<int64_t>(1, (tap_units > 0 ? tap_units : kWgmTapUnits) / taps);
    return (int)std::max(lo, std::min(want, std::max<int64_t>(1, P / 512)));
  }
  const int64_t chunks = P / 64, units = (int64_t)(d.Cin / 16) * (d.Cout / 16 / wgrad_s1_nco(v));
  const int cpw = chunks_per_wave > 0 ? chunks_per_wave : kWgmCpw;
  int64_t ns = std::max<int64_t>(1, chunks / ((int64_t)kFW * cpw));
  if (chunks_per_wave <= 0) {
    // small batches: more, shorter splits (down to one chunk per wave) until the job has kWgmMinUnits
    // workgroups -- a job takes as long as one workgroup's serial chunk loop
    while (ns * units < kWgmMinUnits && 2 * ns * kFW <= chunks) ns *= 2;
  }
  ns = std::max(ns, (chunks + kFW * 1024 - 1) / (kFW * 1024));  // <= 65536 pixels per wave
  while (chunks % ns) --ns;
  return (int)ns;
}

extern "C" int lbt_conv_wgrad_many_i8(const lbt_wgrad_job* jobs, int32_t njobs, void* stream) {
  if (njobs < 0 || (njobs > 0 && !jobs)) return LBT_EINVAL;
  for (int i = 0; i < njobs; ++i) {  // every job checked before anything is queued
    WgradArgs wa;
    uint32_t blocks = 0;
    int32_t fast = 0;
    const int e = wgrad_many_setup(jobs[i], wa, blocks, fast);
    if (e) return e;
  }
  for (int base = 0; base < njobs; base += kMaxWJobs) {
    WgradMany m{};
    const int n = njobs - base < kMaxWJobs ? njobs - base : kMaxWJobs;
    uint64_t total = 0;
    for (int i = 0; i < n; ++i) {
      uint32_t blocks = 0;
      wgrad_many_setup(jobs[base + i], m.j[i], blocks, m.fast[i]);
      m.start[i] = (uint32_t)total;
      total += blocks;
    }
    if (total >= 0x7fffffffull) return LBT_EINVAL;
    m.start[n] = (uint32_t)total;
    m.n = n;
    hipLaunchKernelGGL(conv_wgrad_many_kernel, dim3((unsigned)total), dim3(kFW * 64), 0, (hipStream_t)stream, m);
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
  }
  return 0;
}

extern "C" int lbt_conv_stem_bwd(const lbt_chain_bwd_b* b, const int16_t* x, lbt_conv_desc d, int32_t* slab,
                                 int32_t nshard, void* stream);

// lbt_conv_wgrad_many_i8(jobs) then lbt_conv_stem_bwd(b, x, d, slab, nshard) with the stem's row
// blocks riding in the batched launch (two per workgroup): as its FIRST workgroups by default (measured
// 0.9 us faster), as its last with LBT_STEM_FIRST=0; the same results (integer atomics). A batch too large for one launch, or an odd number of stem row blocks, runs as the two calls.
extern "C" int lbt_conv_wgrad_many_stem_i8(const lbt_wgrad_job* jobs, int32_t njobs, const lbt_chain_bwd_b* b,
                                           const int16_t* x, lbt_conv_desc d, int32_t* slab, int32_t nshard,
                                           void* stream) {
  if (njobs < 0 || (njobs > 0 && !jobs) || !b || !x || !slab || nshard <= 0) return LBT_EINVAL;
  const int64_t M = (int64_t)d.N * d.Ho * d.Wo;
  if (M <= 0 || !stem_bwd_shape_ok(b, d)) return M <= 0 ? lbt_conv_wgrad_many_i8(jobs, njobs, stream) : LBT_EINVAL;
  const int64_t rblocks = M / kSbPixels, pairs = rblocks / 2;
  // int32 shard totals stay exact: <= 31 row blocks per shard (stem.hip lbt_conv_stem_wgrad)
  if (njobs > kMaxWJobs || rblocks % 2 || (pairs + nshard - 1) / nshard * 2 > 31) {
    const int e = lbt_conv_wgrad_many_i8(jobs, njobs, stream);
    return e ? e : lbt_conv_stem_bwd(b, x, d, slab, nshard, stream);
  }
  WgradMany m{};
  uint64_t total = 0;
  for (int i = 0; i < njobs; ++i) {  // every job checked before anything is queued
    uint32_t blocks = 0;
    const int e = wgrad_many_setup(jobs[i], m.j[i], blocks, m.fast[i]);
    if (e) return e;
    m.start[i] = (uint32_t)total;
    total += blocks;
  }
  m.start[njobs] = (uint32_t)total;
  m.n = njobs;
  if (total + pairs >= 0x7fffffffull) return LBT_EINVAL;
  StemBwdArgs st;
  st.b = *b; st.x = x; st.d = d; st.K = d.KH * d.KW * d.Cin; st.slab = slab; st.nshard = nshard;
  // stem blocks first (A/B on one box, isolated launch: 34.2 / 34.3 us vs 35.0 / 35.2 us placed last);
  // LBT_STEM_FIRST=0 places them last
  static const int stem_first = !(getenv("LBT_STEM_FIRST") != nullptr && getenv("LBT_STEM_FIRST")[0] == '0');
  hipLaunchKernelGGL(conv_wgrad_many_stem_kernel, dim3((unsigned)(total + pairs)), dim3(kFW * 64), 0,
                     (hipStream_t)stream, m, st, (uint32_t)pairs, stem_first);
  return (int)hipGetLastError();
}

extern "C" int lbt_conv_wgrad_reduce(const int32_t* slab, int32_t nsplit, int32_t K, int32_t Cout, int32_t x_u8off,
                                     const int64_t* gcolsum, lbt_qdesc qx, lbt_qdesc qg, const float* w, float wd2,
                                     float* dw, void* stream) {
  const int64_t total = (int64_t)K * Cout;
  const int64_t blocks = (total + 31) / 32;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, slab, nsplit, K,
                     Cout, x_u8off, gcolsum, qx, qg, w, wd2, dw, nullptr);
  return (int)hipGetLastError();
}
extern "C" int lbt_conv_wgrad_reduce_x(const int32_t* slab, int32_t nsplit, int32_t K, int32_t Cout, int32_t x_u8off,
                                       const int64_t* gcolsum, int64_t* num, void* stream) {
  if (!num || nsplit <= 0 || K <= 0 || Cout <= 0) return LBT_EINVAL;
  const int64_t blocks = ((int64_t)K * Cout + 31) / 32;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, slab, nsplit, K,
                     Cout, x_u8off, gcolsum, lbt_qdesc{}, lbt_qdesc{}, nullptr, 0.f, nullptr, (long long*)num);
  return (int)hipGetLastError();
}

// Diagnostics: resident workgroups per CU of a few conv GEMM variants (hipOccupancy API), written
// to out[0..n): fwd<CS1,NT1>, dgrad+A<CS1,NT1,26>, dgrad<CS4,NT2>, dgrad+A<CS2,NT2,26>, wgrad<1>.
extern "C" int lbt_diag_occupancy(int32_t* out, int32_t n) {
  const void* k[5] = {reinterpret_cast<const void*>(&conv_gemm_kernel<MODE_FWD, 1, 1, 0, 1, false>),
                      reinterpret_cast<const void*>(&conv_gemm_kernel<MODE_DGRAD, 1, 1, 26, 1, false>),
                      reinterpret_cast<const void*>(&conv_gemm_kernel<MODE_DGRAD, 4, 2, 0, 1, false>),
                      reinterpret_cast<const void*>(&conv_gemm_kernel<MODE_DGRAD, 2, 2, 26, 1, false>),
                      reinterpret_cast<const void*>(&conv_wgrad_kernel<1>)};
  for (int i = 0; i < n && i < 5; ++i) {
    int b = -1;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, k[i], kThreads, 0) != hipSuccess) b = -1;
    out[i] = b;
  }
  return 0;
}
