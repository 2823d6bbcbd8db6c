// conv_wgrad_body.h -- the int8 weight-gradient workgroup body (conv_wgrad_body) with its argument block,
// LDS layout and host-side setup, shared by
//   conv_mfma.hip       conv_wgrad_kernel, dgrad_wgrad_kernel and the batched conv_wgrad_many kernels, and
//   conv_fused_bwd.hip  conv_bwd_kernel's deferred weight-gradient job (WCS != 0).
#pragma once
#include "conv_epilogue.h"
#include "lds_tr.h"

namespace {
using namespace lbt;

// dW[tap][ci][co] = sum_p X[p shifted by tap][ci] * G[p][co]: GEMM rows = ci, cols = co, k = pixels.
// grid (nsplit, taps, Cout/16): workgroup = one tap, one 16-channel co slice, a pixel range; each
// wave walks 64-pixel chunks. A lane loads one pixel's 16-byte channel slices (X: CSI of them,
// G: one) and stores them as rows of [pixel][16 B] LDS images (one ds_write_b128 each); the MFMA
// fragments -- 16 consecutive pixels of one channel -- come back with the gfx950 transposing read
// ds_read_b64_tr_b8 (probed: in a 16-lane group, lane i receives byte i of the 8 rows formed by
// lane pairs 2r, 2r+1). Each workgroup adds its exact int32 partial [CI][16] into shard
// (split % nshard) of a zeroed slab[nshard][tap][ci][co] for the batched reduce.
constexpr int kWP = 64;  // pixels per wave chunk

struct WgradArgs {
  const int8_t* xq;
  const int8_t* gq;
  lbt_conv_desc d;
  int x_fill;
  int32_t* slab;
  int64_t P;
  int nsplit, nshard;
};

// LDS of one wgrad workgroup: per wave an X image [CSI][64 px][16 B] and a G image [64 px][16 B],
// then the per-wave partials [4][CI][16]
template <int CSI, int NW = 4>
struct WgradShared {
  int8_t lds[NW][(CSI + 1) * kWP * 16];
  int red[NW][CSI * 16 * 16];
};

// NW waves per workgroup (4 in the wgrad / dgrad_wgrad kernels, 8 in conv_bwd_kernel)
template <int CSI, int NW = 4>
__device__ __forceinline__ void conv_wgrad_body(const WgradArgs& wa, uint32_t bid, WgradShared<CSI, NW>& sm) {
  const int8_t* __restrict__ xq = wa.xq;
  const int8_t* __restrict__ gq = wa.gq;
  const lbt_conv_desc& d = wa.d;
  const int x_fill = wa.x_fill, nsplit = wa.nsplit, nshard = wa.nshard;
  int32_t* __restrict__ slab = wa.slab;
  const int64_t P = wa.P;
  constexpr int CI = CSI * 16;
  auto& lds = sm.lds;
  auto& red = sm.red;
  LBT_TS(0);
  const int lane = threadIdx.x & 63, wave = wave_id();
  const int r = lane & 15, kg = lane >> 4;
  // XCD-aware unit order: workgroups are dealt round-robin over the 8 XCDs, so unit u of the
  // split-major order (split, tap, co-slice) goes to linear block (u % chunk) * 8 + u / chunk:
  // all taps / co-slices of one pixel split -- which re-read the same G and X bytes -- share one
  // XCD's L2 (speed only; any order gives the same integer sums).
  const int ntap = d.KH * d.KW, ncos = d.Cout >> 4, total = nsplit * ntap * ncos;
  const int chunk = (total + 7) >> 3;
  const int u = (int)(bid & 7) * chunk + (int)(bid >> 3);
  if (u >= total) return;
  const int split = u / (ntap * ncos), urem = u - split * (ntap * ncos);
  const int tap = urem / ncos, cso = urem - tap * ncos;
  const int kh = tap / d.KW, kw = tap - kh * d.KW;
  int8_t* Xi = lds[wave];
  int8_t* Gi = lds[wave] + CSI * kWP * 16;
  const int64_t per = (P + nsplit - 1) / nsplit;
  const int64_t p0 = (int64_t)split * per;
  const int64_t p1 = p0 + per < P ? p0 + per : P;
  const uint32_t HWo = (uint32_t)d.Ho * d.Wo;

  v4i acc[CSI];
#pragma unroll
  for (int a = 0; a < CSI; ++a) acc[a] = v4i{0, 0, 0, 0};

  // chunks are interleaved across the NW waves of the block, two in flight per wave: chunk k + 2's
  // loads are issued while chunk k is computed. Every load is unconditional (a chunk past the end has
  // no valid pixel: clamped addresses, zero gradient), so the compiler's vmcnt waits count exactly the
  // loads issued since instead of waiting for all of them (each chunk then paid a memory round trip:
  // the strided jobs' 32 chunks per wave took ~23 us of the batched launch, profiles/round6/budget)
  struct Chunk {
    v4i xs[CSI], g;
    bool xv, pv;
  };
  // whole-row chunks (the ResNet shapes: 64-pixel chunks of whole output rows of one image, aligned
  // splits): the lane's row / column within a chunk are chunk-invariant and the chunk's image and first
  // row wave-uniform -- no per-lane divisions per chunk
  const bool rows64 = 64 % d.Wo == 0 && HWo % 64 == 0 && per % 64 == 0 && p0 % 64 == 0;
  const int lrow = rows64 ? lane / d.Wo : 0, lcol = rows64 ? lane - lrow * d.Wo : 0;
  auto fetch = [&](int64_t c0, Chunk& b) {
    const int64_t p = c0 + lane;
    const bool pv = p < p1;
    const uint32_t pu = (uint32_t)(pv ? p : p0);  // P < 2^31 (launcher)
    uint32_t n;
    int oh, ow;
    if (rows64) {  // wave-uniform branch
      const uint32_t cu = (uint32_t)(c0 < p1 ? c0 : p0);
      n = cu / HWo;
      oh = (int)((cu - n * HWo) / (uint32_t)d.Wo) + lrow;
      ow = lcol;
    } else {
      n = pu / HWo;
      const uint32_t rem = pu - n * HWo;
      oh = (int)(rem / (uint32_t)d.Wo);
      ow = (int)(rem - (uint32_t)oh * (uint32_t)d.Wo);
    }
    const int ih = oh * d.SH + kh - d.PT, iw = ow * d.SW + kw - d.PL;
    const bool xv = pv && (unsigned)ih < (unsigned)d.H && (unsigned)iw < (unsigned)d.W;
    // all loads first (clamped addresses, no branches), fills selected afterwards
    const int8_t* xp = xq + (xv ? ((((int64_t)n * d.H + ih) * d.W + iw) * CI) : 0);
#pragma unroll
    for (int cs = 0; cs < CSI; ++cs) b.xs[cs] = *reinterpret_cast<const v4i*>(xp + cs * 16);
    b.g = *reinterpret_cast<const v4i*>(gq + (int64_t)pu * d.Cout + cso * 16);
    b.xv = xv;
    b.pv = pv;
  };
  auto consume = [&](Chunk& b, int64_t cnext) {
    const int xf = b.pv ? x_fill : 0;
#pragma unroll
    for (int cs = 0; cs < CSI; ++cs)
      *reinterpret_cast<v4i*>(Xi + (cs * kWP + lane) * 16) = b.xv ? b.xs[cs] : v4i{xf, xf, xf, xf};
    *reinterpret_cast<v4i*>(Gi + lane * 16) = b.pv ? b.g : v4i{0, 0, 0, 0};
    // the images are read by other lanes of the same wave only: a wave's LDS instructions execute in
    // issue order, so only the compiler must keep the reads after the writes
    asm volatile("" ::: "memory");
    fetch(cnext, b);
    const v4i bfrag = tr_frag(Gi, 16 * kg, lane);
#pragma unroll
    for (int a = 0; a < CSI; ++a) {
      const v4i afrag = tr_frag(Xi + a * kWP * 16, 16 * kg, lane);
      acc[a] = __builtin_amdgcn_mfma_i32_16x16x64_i8(afrag, bfrag, acc[a], 0, 0, 0);
    }
    asm volatile("" ::: "memory");  // the next chunk's stores after these reads (in-order LDS)
  };
  const int64_t cw = p0 + (int64_t)wave * kWP, cstep = (int64_t)NW * kWP;
  const int64_t nch = p1 > cw ? (p1 - cw + cstep - 1) / cstep : 0;  // this wave's chunks
  if (nch > 0) {
    Chunk b0, b1;
    fetch(cw, b0);
    fetch(cw + cstep, b1);
    for (int64_t k = 0; k < nch; k += 2) {
      consume(b0, cw + (k + 2) * cstep);
      consume(b1, cw + (k + 3) * cstep);
    }
  }
  LBT_TS(1);
  // acc[a] element i: row = a*16 + 4*kg + i (ci), col = r (co within the slice)
#pragma unroll
  for (int a = 0; a < CSI; ++a)
#pragma unroll
    for (int i = 0; i < 4; ++i) red[wave][(a * 16 + kg * 4 + i) * 16 + r] = acc[a][i];
  __syncthreads();
  LBT_TS(2);
  int32_t* dst = slab + ((int64_t)(split % nshard) * (d.KH * d.KW) + tap) * CI * d.Cout + cso * 16;
  for (int i = threadIdx.x; i < CI * 16; i += NW * 64) {
    const int ci = i >> 4, co = i & 15;
    int v = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) v += red[w][i];
    if (v) LBT_GADD(&dst[(int64_t)ci * d.Cout + co], v);  // integer atomics: exact, order-independent
  }
  LBT_TS(3);
}

// The wgrad launch of one conv: its argument block and grid (a multiple of 8 workgroups).
inline int wgrad_setup(const int8_t* xq, int32_t x_u8off, const int8_t* gq, const lbt_conv_desc& d, int32_t* slab,
                int32_t nsplit, int32_t nshard, WgradArgs& wa, uint32_t& blocks) {
  if (!desc_ok(d) || d.Cin % 16 || d.Cout % 16 || nsplit <= 0 || nshard <= 0 || nshard > nsplit) return LBT_EINVAL;
  if (d.Cin / 16 != 1 && d.Cin / 16 != 2 && d.Cin / 16 != 4 && d.Cin / 16 != 8) return LBT_EINVAL;
  const int64_t P = (int64_t)d.N * d.Ho * d.Wo;
  if (P >= ((int64_t)1 << 31)) return LBT_EINVAL;
  // int32 shard totals: the pixels of one shard times |x*g| <= 255*128 stay below 2^31
  if ((P + nsplit - 1) / nsplit * ((nsplit + nshard - 1) / nshard) > 65536) return LBT_EINVAL;
  const int64_t units = (int64_t)nsplit * d.KH * d.KW * (d.Cout / 16);
  if (units >= ((int64_t)1 << 30)) return LBT_EINVAL;
  wa = WgradArgs{xq, gq, d, x_u8off ? (int)0x80808080u : 0, slab, P, nsplit, nshard};
  blocks = (uint32_t)((units + 7) / 8 * 8);
  return 0;
}

}  // namespace
