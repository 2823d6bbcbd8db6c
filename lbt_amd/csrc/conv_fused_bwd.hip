// conv_fused_bwd.hip -- the fused conv backward kernels (conv_fused.h's scaffold).
#include "conv_fused.h"
#include "conv_wgrad_body.h"

using namespace lbt;

LBT_TRACE_SETTER(conv_bwd)

// ============================================================================ fused conv backward
// lbt_conv_bwd_fused_i8: one stride-1 3x3 conv's backward with both neighbouring BN passes in ONE
// launch. A dgrad workgroup owns tile_rows(CS) image rows of one sample:
//   phase 1  pass B of the BN after the conv (bn.hip chain_bwd_b_kernel's arithmetic) over the rows
//            plus a one-pixel halo -> int8 gq codes in LDS; owned pixels also store gq (the weight
//            gradient's operand), count overflows and add the gq channel sums
//   phase 2  dgrad on v_mfma_i32_16x16x64_i8 with every A fragment a 16-byte ds_read of the LDS
//            gq image (the 9 taps never go back to memory) -> fp32 tile in LDS
//   phase 3  pass A of the BN before the conv (chain_bwd_a_kernel's arithmetic) over the tile, one
//            channel quad per thread with vector loads / stores
// Workgroups [0, nwg) run a weight-gradient job instead (conv_wgrad_body): the deferred wgrad of the
// conv of the previous launch.
namespace {

struct ConvBwdArgs {
  lbt_chain_bwd_b b;
  const int8_t* wd;
  int ks, nslices, w4;
  lbt_qdesc qw;
  int H, W;
  const float* add_src;
  lbt_chain_bwd_a a;
};

template <int C, int TH, int WB>
struct BwdShared {
  int8_t w[WB];                                  // the dgrad weight image (WImg)
  int8_t gq[(TH + 2) * (512 / C + 2) * C];   // halo image [(TH+2)][(W+2)][C], W*C == 512
  float tile[TH * (512 / C) * (C + 4)];       // dgrad outputs [TH*W][C+4] (padded rows)
  float pb[2 * C];                               // pass-B constants mg, mgx per channel
  int part[kBNW][(2 * 4 + 2) * C];               // per wave: pass-A sums per branch, gq sums
  int cnt[kBNW * 2 * 5];                         // counters: 5 quantisers x waves
};

template <int CS, int CF, int NB, bool W4, int WCS, int TH = tile_rows(CS)>
__global__ __launch_bounds__(kBThreads, (CS == 4 && TH >= 4) ? 2 : 4) void conv_bwd_kernel(ConvBwdArgs p, WgradArgs wa, uint32_t nwg) {
  using T = FusedTile<CS, TH>;
  constexpr int C = T::C, C4 = T::C4, NT = T::NT, W = T::W, Wp = T::Wp, kMaxKS = T::kMaxKS;
  constexpr int kBIt = T::kBIt, NPR = T::NPR, NQ = T::NQ, J = T::J;
  constexpr int WC = WCS ? WCS : 1;
  using WI = WImg<C, 4 * kMaxKS, W4>;
  union Smem {
    BwdShared<C, TH, WI::kBytes> b;
    WgradShared<WC, kBNW> w;
  };
  __shared__ __attribute__((aligned(16))) Smem sm;
  if (WCS != 0 && blockIdx.x < nwg) {
    conv_wgrad_body<WC, kBNW>(wa, blockIdx.x, sm.w);
    return;
  }
  BwdShared<C, TH, WI::kBytes>& sh = sm.b;
  LBT_TS(0);
  const lbt_chain_bwd_b& B = p.b;
  const lbt_chain_bwd_a& A = p.a;
  const int H = p.H;
  const uint32_t bid = blockIdx.x - nwg;
  const int tpi = H / TH;
  const int n = (int)(bid / (uint32_t)tpi), row0 = (int)(bid - (uint32_t)n * tpi) * TH;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, kg = lane >> 4;
  const int cq = (tid % C4) * 4;  // this thread's channel quad (512 % C4 == 0: fixed over its groups)
  const int64_t img = (int64_t)n * H * W * C;

  // ---------------- the pass-B statistics' shard sums first (they gate the first barrier): waves
  // w < C / 16 each own 16 channels (SG, SGQ: sums 2 and 3 of the BN's [shard][4C] table): lane l reads
  // channel w*16 + (l & 15) of shards 8*(l >> 4) .. +7, so every load instruction covers 4 shards x 16
  // consecutive channels (128-byte rows); rows_total64 adds the wave's four lane rows.
  static_assert(LBT_NSHARD == 32 && kBThreads == 512 && C % 16 == 0 && C / 16 <= kBNW, "statistics layout");
  constexpr int kSW = C / 16;  // statistics waves
  long long sv[8][2];
  if (wave < kSW) {  // uniform per wave
    const int64_t* ps = B.sums + (int64_t)(8 * (lane >> 4)) * 4 * C + wave * 16 + (lane & 15);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      sv[i][0] = ps[(int64_t)i * 4 * C + 2 * C];
      sv[i][1] = ps[(int64_t)i * 4 * C + 3 * C];
    }
  }
  LBT_TSS(1);  // the statistics loads issued
  // then every load that does not depend on the sums
  // phase-1 operands: G / q codes and the output quantiser's noise over the halo rows inside the image
  // (rows ylo .. yhi, whole rows of W pixels: group g is pixel g / C4 of them; halo_pad_fill)
  const int ylo = row0 > 0 ? row0 - 1 : 0, yhi = row0 + TH < H ? row0 + TH : H - 1;
  const int ngrp = (yhi - ylo + 1) * W * C4;  // a multiple of 128: whole waves
  int Gv[kBIt], Qv[kBIt];
  float4 Uv[kBIt];
#pragma unroll
  for (int it = 0; it < kBIt; ++it) {
    const int g = tid + it * kBThreads;
    const uint32_t off = g < ngrp ? (uint32_t)((ylo * W + g / C4) * C + cq) : 0u;
    Gv[it] = ld_i8x4(B.G, img + off);
    Qv[it] = ld_i8x4(B.qn_codes, img + off);
    Uv[it] = ld_f32x4(B.qo.noise, off);
  }
  // the phase-2 B operands (the dgrad weight image, ks == 4 * kMaxKS: host check), for LDS (WImg)
  v4i wimg[WI::kIt];
  WI::load(p.wd, wimg);
  float mu[4], sg[4], gam[2][4], bet[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    mu[k] = B.ms[cq + k];
    sg[k] = B.ms[C + cq + k];
#pragma unroll
    for (int b = 0; b < NB; ++b) gam[b][k] = (b == 0 ? A.b1 : A.b2).gb[cq + k];
    bet[k] = A.b1.gb[C + cq + k];
  }
  const QState sgq = qstate(B.qng), sn = qstate(B.qn), so = qstate(B.qo);
  QState qrg[2], qng[2];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    qrg[b] = qstate((b == 0 ? A.b1 : A.b2).qrg);
    qng[b] = qstate((b == 0 ? A.b1 : A.b2).qng);
  }
  const float r_inv = (CF & kAMaskR) ? qstate(A.b1.qr).inv_m : 0.f;
  const float scale = ldexpf(1.0f, -(frac_exp(B.qo) + frac_exp(p.qw)));
  LBT_TSS(2);  // every other load issued, the descriptors read

  // ---------------- pass-B statistics: the shard sums (loaded first, above) added per lane, then over
  // the statistics wave's four lane rows; lanes < 16 finish their channel in double exactly as
  // chain_bwd_b_kernel
  if (wave < kSW) {
    long long SGi = 0, SGQi = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      SGi += sv[i][0];
      SGQi += sv[i][1];
    }
    SGi = rows_total64(SGi);
    SGQi = rows_total64(SGQi);
    const int c = wave * 16 + (lane & 15);
    if (lane < 16) {
      const double s = (double)sn.inv_m, gsc = (double)sgq.inv_m, nn = (double)B.n;
      const double SG = (double)SGi, SGQ = (double)SGQi;
      const float m = B.ms[c], sig = B.ms[C + c];
      sh.pb[c] = (float)(gsc * SG / nn);
      sh.pb[C + c] = (float)(gsc * (s * SGQ - (double)m * SG) / (nn * (double)sig));
    }
  }
  LBT_TSS(3);  // the statistics finished
  __syncthreads();
  LBT_TSB(1);
  float rmg[4], rmgx[4];
  Recip rsg[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    rmg[k] = sh.pb[cq + k];
    rmgx[k] = sh.pb[C + cq + k];
    rsg[k] = recip(sg[k]);
  }
  pf2 mu2[2], sg2[2], rsc2[2], rmg2[2], rmgx2[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    mu2[h] = pk(mu[2 * h], mu[2 * h + 1]);
    sg2[h] = pk(rsg[2 * h].y, rsg[2 * h + 1].y);
    rsc2[h] = pk(rsg[2 * h].rc, rsg[2 * h + 1].rc);
    rmg2[h] = pk(rmg[2 * h], rmg[2 * h + 1]);
    rmgx2[h] = pk(rmgx[2 * h], rmgx[2 * h + 1]);
  }

  // ---------------- phase 1: pass B over the rows + halo -> LDS gq image
  // the wave index as a scalar: the wave-uniform loop exits and halo tests below are then scalar branches
  // and selects, so the overflow totals (ov_count2) never pass through a VGPR
  const int wu = __builtin_amdgcn_readfirstlane(wave);
  int ovq = 0;
  int s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
#pragma unroll
  for (int it = 0; it < kBIt; ++it) {
    if (it * kBThreads + wu * 64 >= ngrp) break;  // uniform per wave (ngrp % 64 == 0: every lane has a group)
    const int g = tid + it * kBThreads;
    const int ry = g / (W * C4), x = g / C4 - ry * W;
    const int y = ylo + ry, hy = y - row0 + 1;
    const int pix = hy * Wp + x + 1;  // the pixel's cell of the LDS halo image
    const bool own = hy >= 1 && hy <= TH;
    // a wave's 64 groups lie in one row (W * C4 == 128): its own-ness from the wave's first group, a scalar
    const int hyw = ylo + (it * kBThreads + wu * 64) / (W * C4) - row0 + 1;
    const int nanw = hyw >= 1 && hyw <= TH ? 0 : kOvNan;
    const float T1 = ov_thr(nanw, so.L), T2 = ov_thr(nanw, so.Lh);
    int G[4], q[4], c[4];
    unpack4_i8(Gv[it], G);
    unpack4_i8(Qv[it], q);
    const pf2 u[2] = {pk(Uv[it].x, Uv[it].y), pk(Uv[it].z, Uv[it].w)};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const pf2 x1 = pcvt(q[2 * h], q[2 * h + 1]) * sn.inv_m;
      const pf2 x2 = x1 - mu2[h];
      const pf2 xh = pdiv_nz(x2, sg2[h], rsc2[h]);
      const pf2 gh = pcvt(G[2 * h], G[2 * h + 1]) * sgq.inv_m;
      const pf2 t1 = gh - rmg2[h];
      const pf2 t2 = xh * rmgx2[h];
      const pf2 dx = pdiv_nz(t1 - t2, sg2[h], rsc2[h]);
      const pf2 xm = dx * so.m;
      ov_count2(xm, T1, T2, ovq);
      const pf2 fl = qfloor2(so, xm, u[h]);
      c[2 * h] = (int)fl.x;
      c[2 * h + 1] = (int)fl.y;
    }
    *reinterpret_cast<int*>(sh.gq + pix * C + cq) = pack4_i8(c);
    if (own) {
      st_out(B.gq + img + (uint32_t)((y * W + x) * C + cq), pack4_i8(c));
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        s1[k] += c[k];
        s2[k] += c[k] * c[k];
      }
    }
  }
  halo_pad_fill<C, TH>(sh.gq, row0, H, 0);  // outside the image: the conv's zero padding
  WI::store(sh.w, wimg);
  __syncthreads();
  LBT_TSB(2);

  // phase-3 operands (addend, mask source, R / qn codes and both quantisers' noise per branch),
  // issued now: they land while the MFMAs run, and phase 1's registers are free
  float4 av[J], ymv[J], urg[NB][J], ung[NB][J];
  int Rv[NB][J], qnv[NB][J];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int q3 = tid + j * kBThreads;
    const int pix = (q3 < NQ ? q3 : 0) / C4;  // (2-row tiles: the idle threads load the tile's first quad)
    const uint32_t off = (uint32_t)(row0 * W * C + pix * C + cq);  // tile rows are consecutive pixels
    av[j] = p.add_src ? ld_f32x4(p.add_src, img + off) : make_float4(0.f, 0.f, 0.f, 0.f);
    if (CF & kAYMask) ymv[j] = ld_f32x4(A.y_mask, img + off);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const lbt_bwd_branch& Bb = b == 0 ? A.b1 : A.b2;
      Rv[b][j] = ld_i8x4(Bb.R, img + off);
      qnv[b][j] = ld_i8x4(Bb.qn_codes, img + off);
      urg[b][j] = ld_f32x4(Bb.qrg.noise, off);
      ung[b][j] = ld_f32x4(Bb.qng.noise, off);
    }
  }

  // ---------------- phase 2: dgrad from the LDS image, (m-tile, n-tile) pair wave + 8 pi (as
  // conv_fwd_fused_kernel's phase 2 with the taps mirrored)
#pragma unroll
  for (int pi = 0; pi < (NPR + 7) / 8; ++pi) {
    const int pr = wave + 8 * pi;
    if (NPR % 8 && pr >= NPR) break;  // uniform per wave
    const int mt = pr / NT, nt = pr - mt * NT;
    const int m = mt * 16 + r;
    const int ly = m / W, px = m - ly * W;
    const int8_t* base = sh.gq + ((ly + 2) * Wp + px + 2) * C;
    v4i acc = v4i{0, 0, 0, 0};
    const int col = nt * 16 + r;
#pragma unroll
    for (int kk = 0; kk < kMaxKS; ++kk) {
      const int s = kk * 4 + kg;  // the k-slice this lane group supplies: (tap, 16-channel slice)
      const int tap = s / CS, cs = s - tap * CS;
      const int kh = tap / 3, kw = tap - kh * 3;
      v4i a = *reinterpret_cast<const v4i*>(base - (kh * Wp + kw) * C + cs * 16);
      if (s >= 9 * CS) a = v4i{0, 0, 0, 0};  // zero padding of the k dimension
      acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, WI::frag(sh.w, col, s), acc, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) sh.tile[(mt * 16 + 4 * kg + i) * (C + 4) + nt * 16 + r] = (float)acc[i] * scale;
  }
  __syncthreads();
  LBT_TSB(3);

  // ---------------- phase 3: pass A over the tile (conv_bwd2_kernel's phase 3 is a copy of this one)
  int ov[2][2] = {{0, 0}, {0, 0}};  // [branch][qrg | qng]
  int acc3[NB][4][4];
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int k = 0; k < 4; ++k) acc3[b][s][k] = 0;
  const bool has_add = p.add_src != nullptr;
  pf2 gam2a[NB][2], bet2a[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int b = 0; b < NB; ++b) gam2a[b][h] = pk(gam[b][2 * h], gam[b][2 * h + 1]);
    bet2a[h] = pk(bet[2 * h], bet[2 * h + 1]);
  }
#pragma unroll
  for (int j = 0; j < J; ++j) {
    if (NQ % kBThreads && wu * 64 + j * kBThreads >= NQ) break;  // uniform per wave (NQ % 64 == 0)
    const int pix = (tid + j * kBThreads) / C4;
    const uint32_t off = (uint32_t)(row0 * W * C + pix * C + cq);
    const float4 t = *reinterpret_cast<const float4*>(sh.tile + pix * (C + 4) + cq);
    pf2 g[2] = {pk(t.x, t.y), pk(t.z, t.w)};
    if (has_add) {
      g[0] = g[0] + pk(av[j].x, av[j].y);
      g[1] = g[1] + pk(av[j].z, av[j].w);
    }
    int R1[4];
    unpack4_i8(Rv[0][j], R1);
    if (CF & kAYMask) {
      const float ym[4] = {ymv[j].x, ymv[j].y, ymv[j].z, ymv[j].w};
#pragma unroll
      for (int h = 0; h < 2; ++h)
        g[h] = pk(ym[2 * h] > 0.f ? g[h].x : 0.f, ym[2 * h + 1] > 0.f ? g[h].y : 0.f);
    } else if (CF & kAMaskR) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const pf2 xr = pcvt(R1[2 * h], R1[2 * h + 1]) * r_inv;
        const pf2 m1 = xr * gam2a[0][h];
        const pf2 yv = m1 + bet2a[h];
        g[h] = pk(yv.x > 0.f ? g[h].x : 0.f, yv.y > 0.f ? g[h].y : 0.f);
      }
    }
    if (CF & kAGmask) st_out4(A.gmask_out, (uint32_t)(img + off), make_float4(g[0].x, g[0].y, g[1].x, g[1].y));
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const lbt_bwd_branch& Bb = b == 0 ? A.b1 : A.b2;
      int R[4], qn[4], Gc[4];
      unpack4_i8(Rv[b][j], R);
      unpack4_i8(qnv[b][j], qn);
      const pf2 ur[2] = {pk(urg[b][j].x, urg[b][j].y), pk(urg[b][j].z, urg[b][j].w)};
      const pf2 un[2] = {pk(ung[b][j].x, ung[b][j].y), pk(ung[b][j].z, ung[b][j].w)};
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const pf2 xm = g[h] * qrg[b].m;
        ov_count2(xm, qrg[b].L, qrg[b].Lh, ov[b][0]);
        const pf2 f1 = qfloor2(qrg[b], xm, ur[h]);  // G2 codes
        const pf2 gh = f1 * qrg[b].inv_m;
        const pf2 d = gh * gam2a[b][h];
        const pf2 dm = d * qng[b].m;
        ov_count2(dm, qng[b].L, qng[b].Lh, ov[b][1]);
        const pf2 f2c = qfloor2(qng[b], dm, un[h]);  // Gc codes
        const int G2[2] = {(int)f1.x, (int)f1.y};
        Gc[2 * h] = (int)f2c.x;
        Gc[2 * h + 1] = (int)f2c.y;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int k = 2 * h + i;
          acc3[b][0][k] += G2[i] * R[k];
          acc3[b][1][k] += G2[i];
          acc3[b][2][k] += Gc[k];
          acc3[b][3][k] += Gc[k] * qn[k];
        }
      }
      st_out(Bb.gout + img + off, pack4_i8(Gc));
    }
  }

  // ---------------- channel sums: wave butterfly -> this wave's LDS slots (plain stores, no LDS
  // atomics); counters; one barrier; the waves' slots summed and flushed
  {
    // lanes l, l + C4, ... hold the same channels (C4 <= 16 divides 64); after chan_scatter4 the
    // lanes (lane & 15) < C4 of row lane >> 4 hold channel cq + (lane >> 4)
    const bool own = (lane & 15) < C4;
    int* part = sh.part[wave] + cq + (lane >> 4);
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int t = chan_scatter4(acc3[b][s], C4);
        if (own) part[(b * 4 + s) * C] = t;
      }
    const int t1 = chan_scatter4(s1, C4), t2 = chan_scatter4(s2, C4);
    if (own) {
      part[8 * C] = t1;
      part[9 * C] = t2;
    }
  }
  // slots [qo | qrg, qng of branch 1 | qrg, qng of branch 2] (counts_publish sums the kBNW waves)
  ov_stage_w(0, 5, ovq, sh.cnt);
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    ov_stage_w(1 + 2 * b, 5, ov[b][0], sh.cnt);
    ov_stage_w(2 + 2 * b, 5, ov[b][1], sh.cnt);
  }
  __syncthreads();
  LBT_TSB(4);
  counts_publish_nw<kBNW>(0, 5, B.qo, sh.cnt);
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const lbt_bwd_branch& Bb = b == 0 ? A.b1 : A.b2;
    counts_publish_nw<kBNW>(1 + 2 * b, 5, Bb.qrg, sh.cnt);
    counts_publish_nw<kBNW>(2 + 2 * b, 5, Bb.qng, sh.cnt);
  }
  // slot i of [NB*4C pass-A sums | 2C gq sums]: one thread each, the waves' partials in int64
  const int shard = shard_id();
  for (int i = tid; i < (NB * 4 + 2) * C; i += kBThreads) {
    const int slot = i < NB * 4 * C ? i : 8 * C + (i - NB * 4 * C);
    long long v = 0;
#pragma unroll
    for (int w = 0; w < kBNW; ++w) v += sh.part[w][slot];
    if (!v) continue;
    int64_t* dst;
    if (i < NB * 4 * C) {
      const int b = i / (4 * C);
      dst = (b == 0 ? A.b1 : A.b2).sums + (int64_t)shard * 4 * C + (i - b * 4 * C);
    } else {
      if (!B.gcolsum) continue;
      dst = B.gcolsum + (int64_t)shard * 2 * C + (i - NB * 4 * C);
    }
    LBT_GADD((unsigned long long*)dst, (unsigned long long)v);
  }
  LBT_TSB(5);
}

}  // namespace

extern "C" int lbt_conv_bwd_fused_i8(const lbt_conv_bwd* q, void* stream) {
  if (!q) return LBT_EINVAL;
  const lbt_conv_desc& d = q->d;
  const int C = d.Cin;
  if (!desc_ok(d) || d.KH != 3 || d.KW != 3 || d.SH != 1 || d.SW != 1 || d.PT != 1 || d.PB != 1 || d.PL != 1 ||
      d.PR != 1 || d.Ho != d.H || d.Wo != d.W || d.Cout != C || (C != 16 && C != 32 && C != 64) ||
      d.H % tile_rows(C / 16) || d.W * C != 512 || (int64_t)d.N * d.H * 512 >= ((int64_t)1 << 29))
    return LBT_EINVAL;  // (st_out4's 32-bit byte offsets)
  const int CS = C / 16;
  const int64_t inner = (int64_t)d.H * d.W * C;
  const lbt_chain_bwd_b& b = q->b;
  if (!b.G || !b.qn_codes || !b.ms || !b.sums || !b.gq || b.dx || !noise_ok(b.qo) || b.C != C || b.rows != d.N ||
      b.inner != inner)
    return LBT_EINVAL;
  const lbt_chain_bwd_a& a = q->a;
  if (a.C != C || a.rows != d.N || a.inner != inner) return LBT_EINVAL;
  const int f = bwd_a_flags(a);
  if ((f & kAFused) != kAFused) return LBT_EINVAL;
  for (int br = 0; br < (a.has_b2 ? 2 : 1); ++br) {
    const lbt_bwd_branch& Bb = br ? a.b2 : a.b1;
    if (!noise_ok(Bb.qrg) || !noise_ok(Bb.qng) || !Bb.gb) return LBT_EINVAL;
  }
  if (q->ksd != 4 * ((9 * CS + 3) / 4) || !q->wd) return LBT_EINVAL;
  if (q->w4 && q->qw.bits > 4) return LBT_EINVAL;
  if (q->b.qo.bits > 8) return LBT_EINVAL;  // int8 gq codes; the int32 channel sums of q^2 assume |q| <= 2^7
  WgradArgs wa{};
  uint32_t wblocks = 0;
  int wcs = 0;
  if (q->w.slab) {
    const int e = wgrad_setup(q->w.xq, q->w.x_u8off, q->w.gq, q->w.d, q->w.slab, q->w.nsplit, q->w.nshard, wa, wblocks);
    if (e) return e;
    wcs = q->w.d.Cin / 16;
  }
  ConvBwdArgs p;
  p.b = b; p.wd = q->wd; p.ks = q->ksd; p.nslices = 9 * CS; p.w4 = q->w4; p.qw = q->qw;
  p.H = d.H; p.W = d.W; p.add_src = q->add_src; p.a = a;
  const int th = lbt_conv_fused_tile_rows(C, d.N, d.H);
  const int64_t tiles = (int64_t)d.N * (d.H / th);
  if (tiles + wblocks > 0x7fffffff) return LBT_EINVAL;
  const dim3 grid((unsigned)(tiles + wblocks));
  hipStream_t st = (hipStream_t)stream;
  const int nb = a.has_b2 ? 2 : 1;
  // the combinations the fused ResNet plan runs (c2: mask from R1, deferred wgrad of the next
  // block's c1 or none; c1: its consumer's chain, deferred wgrad of the same block's c2)
#define LBT_BW_TH(CS_, CF_, NB_, WCS_, TH_)                                                                 \
  if (q->w4)                                                                                                \
    hipLaunchKernelGGL((conv_bwd_kernel<CS_, CF_, NB_, true, WCS_, TH_>), grid, dim3(kBThreads), 0, st, p, wa, wblocks); \
  else                                                                                                      \
    hipLaunchKernelGGL((conv_bwd_kernel<CS_, CF_, NB_, false, WCS_, TH_>), grid, dim3(kBThreads), 0, st, p, wa, wblocks);
#define LBT_BW(CS_, CF_, NB_, WCS_)                                                                  \
  if (CS == CS_ && f == (CF_) && nb == NB_ && wcs == WCS_) {                                       \
    if (CS_ == 1 && th == 4) {                                                                     \
      LBT_BW_TH(CS_, CF_, NB_, WCS_, (CS_ == 1 ? 4 : tile_rows(CS_)))                              \
    } else if (th == 2) {                                                                          \
      LBT_BW_TH(CS_, CF_, NB_, WCS_, 2)                                                            \
    } else {                                                                                       \
      LBT_BW_TH(CS_, CF_, NB_, WCS_, tile_rows(CS_))                                               \
    }                                                                                              \
    return (int)hipGetLastError();                                                                 \
  }
  // (WCS = 0 everywhere: the plan's LBT_SIDE_WGRAD mode runs each wgrad as a parallel branch)
#define LBT_BW_CS(CS_)                                          \
  LBT_BW(CS_, kAFused | kAMaskR, 1, 0)                          \
  LBT_BW(CS_, kAFused | kAMaskR, 1, CS_)                        \
  LBT_BW(CS_, kAFused | kAYMask | kAGmask, 1, 0)                \
  LBT_BW(CS_, kAFused | kAYMask | kAGmask, 1, CS_)              \
  LBT_BW(CS_, kAFused | kAYMask, 2, 0)                          \
  LBT_BW(CS_, kAFused | kAYMask, 2, CS_)
  LBT_BW_CS(1)
  LBT_BW_CS(2)
  LBT_BW_CS(4)
  LBT_BW(1, kAFused | kAYMask, 1, 0)
  LBT_BW(1, kAFused | kAYMask, 1, 1)
  // a stage's last c2 carrying the wgrad of the next stage's c2 (across the projection block)
  LBT_BW(1, kAFused | kAMaskR, 1, 2)
  LBT_BW(2, kAFused | kAMaskR, 1, 4)
#undef LBT_BW_CS
#undef LBT_BW
#undef LBT_BW_TH
  return LBT_EINVAL;
}

// ============================================================================ fused transition backward
// lbt_conv_bwd2_fused_i8: a projection block's first-conv / shortcut backward (the stage transition)
// in ONE launch -- what lbt_bn_chain_bwd_b_pair + lbt_conv_dgrad2_chain_i8 computed in two:
//   phase 1  pass B of BOTH BNs after the strided convs (conv-1's bn1 and the shortcut BN, at the
//            low resolution Hq x Wq x Cq, Cq = 2C) over the low-res rows the workgroup's dx rows read
//            (plus the one-row halo above that the 3x3/2 conv's SAME padding (top 0, bottom 1)
//            reaches) -> int8 gradient-code images in LDS; owned rows store gq (the weight
//            gradients' operands), count overflows and add the gq channel sums
//   phase 2  dx = dgrad(3x3/2, gq1) + dgrad(1x1/2, gqs) from LDS: each lane's dx pixel takes the
//            taps of its parity (the stride's zero rows read as 0), the two GEMMs in their own
//            accumulators, summed in fp32 in the order the dual dgrad launch used
//   phase 3  pass A of the BN that consumes dx (conv_bwd_kernel's phase 3)
namespace {

struct ConvBwd2Args {
  lbt_chain_bwd_b b1, bs;
  const int8_t* wd1;
  const int8_t* wds;
  lbt_qdesc qw1, qws;
  int H;  // dx rows
  lbt_chain_bwd_a a;
};

template <int C, int TH>
struct Bwd2Shared {
  int8_t g1[(TH / 2 + 1) * 512];   // conv-1's gradient codes, low-res rows q0-1 .. q0+TH/2-1 ([row][Wq][Cq])
  int8_t gs[(TH / 2) * 512];       // the shortcut's, rows q0 .. q0+TH/2-1
  float tile[TH * (512 / C) * (C + 4)];
  float cst[2][5][2 * C];          // per BN (conv-1's, shortcut's): mu, sigma, sigma's rcp refinement, mg, mgx
  int part[kBNW][(2 * 4 + 8) * C]; // per wave: pass-A sums (<= 2 branches x 4C), gq sums (2 x 2Cq)
  int cnt[kBNW * 2 * 6];           // counters: qo1, qos, qrg / qng per branch
};

template <int CS, int CF, int NB, bool W4>
__global__ __launch_bounds__(kBThreads, CS == 1 ? 4 : 2) void conv_bwd2_kernel(ConvBwd2Args p) {
  constexpr int TH = tile_rows(CS);
  using T = FusedTile<CS, TH>;
  constexpr int C = T::C, C4 = T::C4, W = T::W, NT = T::NT, Cq = 2 * C, Cq4 = Cq / 4, CSq = 2 * CS;
  constexpr int Wq = W / 2, J = T::J;  // W * C == Wq * Cq == 512 (host check)
  constexpr int kK1 = (9 * CSq + 3) / 4;  // k-steps of the 3x3/2 dgrad
  constexpr int NG1 = (TH / 2 + 1) * Wq * Cq4, NGS = (TH / 2) * Wq * Cq4;
  constexpr int kIt = (NG1 + NGS + kBThreads - 1) / kBThreads;
  static_assert(NG1 % 64 == 0 && CSq <= 4 && LBT_NSHARD == 32 && 2 * Cq / 16 <= kBNW, "layout");
  __shared__ __attribute__((aligned(16))) Bwd2Shared<C, TH> sh;
  LBT_TS(0);
  const lbt_chain_bwd_a& A = p.a;
  const int H = p.H, Hq = H / 2;
  const uint32_t bid = blockIdx.x;
  const int tpi = H / TH;
  const int n = (int)(bid / (uint32_t)tpi), r0 = (int)(bid - (uint32_t)n * tpi) * TH, q0 = r0 / 2;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, kg = lane >> 4;
  const int cq = (tid % C4) * 4;     // dx channel quad (phase 3)
  const int cqq = (tid % Cq4) * 4;   // low-res channel quad (phase 1)
  const int64_t img = (int64_t)n * H * W * C, imgq = (int64_t)n * Hq * Wq * Cq;

  // ---------------- both BNs' pass-B statistics shard sums first (they gate the first barrier):
  // wave w < 2 * CSq owns 16 channels of BN w / CSq; lane l reads shards 8 (l >> 4) .. + 7
  constexpr int kSW = 2 * CSq;
  long long sv[8][2];
  if (wave < kSW) {
    const lbt_chain_bwd_b& Bb = wave < CSq ? p.b1 : p.bs;
    const int c = (wave % CSq) * 16 + (lane & 15);
    const int64_t* ps = Bb.sums + (int64_t)(8 * (lane >> 4)) * 4 * Cq + c;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      sv[i][0] = ps[(int64_t)i * 4 * Cq + 2 * Cq];
      sv[i][1] = ps[(int64_t)i * 4 * Cq + 3 * Cq];
    }
  }
  // phase-1 operands: G / q codes and the output quantiser's noise of the low-res groups (region 1:
  // conv-1's BN over rows q0-1 .. q0+TH/2-1; region 2: the shortcut BN over rows q0 .. q0+TH/2-1)
  int Gv[kIt], Qv[kIt];
  float4 Uv[kIt];
#pragma unroll
  for (int it = 0; it < kIt; ++it) {
    const int g = tid + it * kBThreads;
    const bool r1 = g < NG1;  // wave-uniform (NG1 % 64 == 0)
    const int gg = r1 ? g : g - NG1;
    const int pix = gg / Cq4, hy = pix / Wq, x = pix - hy * Wq;
    const int y = r1 ? q0 - 1 + hy : q0 + hy;
    const bool in = (r1 || gg < NGS) && (unsigned)y < (unsigned)Hq;
    const uint32_t off = in ? (uint32_t)((y * Wq + x) * Cq + cqq) : 0u;
    const lbt_chain_bwd_b& Bb = r1 ? p.b1 : p.bs;
    Gv[it] = ld_i8x4(Bb.G, imgq + off);
    Qv[it] = ld_i8x4(Bb.qn_codes, imgq + off);
    Uv[it] = ld_f32x4(Bb.qo.noise, off);
  }
  // phase-2 B operands of this wave's n-tile (NT | 8): the 3x3/2 dgrad image and the 1x1/2 one
  v4i bf1[kK1], bfs;
  {
    const int col = (wave % NT) * 16 + r;
#pragma unroll
    for (int kk = 0; kk < kK1; ++kk) {
      if constexpr (W4)
        bf1[kk] = unpack_i4x16(*reinterpret_cast<const v2i*>(p.wd1 + ((int64_t)col * (4 * kK1) + kk * 4 + kg) * 8));
      else
        bf1[kk] = *reinterpret_cast<const v4i*>(p.wd1 + ((int64_t)col * (4 * kK1) + kk * 4 + kg) * 16);
    }
    if constexpr (W4)
      bfs = unpack_i4x16(*reinterpret_cast<const v2i*>(p.wds + ((int64_t)col * 4 + kg) * 8));
    else
      bfs = *reinterpret_cast<const v4i*>(p.wds + ((int64_t)col * 4 + kg) * 16);
  }
  float gam[NB][4], bet[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
#pragma unroll
    for (int b = 0; b < NB; ++b) gam[b][k] = (b == 0 ? A.b1 : A.b2).gb[cq + k];
    bet[k] = A.b1.gb[C + cq + k];
  }
  const QState so1 = qstate(p.b1.qo), sos = qstate(p.bs.qo);
  QState qrg[2], qng[2];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    qrg[b] = qstate((b == 0 ? A.b1 : A.b2).qrg);
    qng[b] = qstate((b == 0 ? A.b1 : A.b2).qng);
  }
  const float r_inv = (CF & kAMaskR) ? qstate(A.b1.qr).inv_m : 0.f;
  const float scale1 = ldexpf(1.0f, -(frac_exp(p.b1.qo) + frac_exp(p.qw1)));
  const float scale2 = ldexpf(1.0f, -(frac_exp(p.bs.qo) + frac_exp(p.qws)));

  // ---------------- pass-B constants of both BNs (chain_bwd_b_kernel's double arithmetic)
  if (wave < kSW) {
    long long SGi = 0, SGQi = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      SGi += sv[i][0];
      SGQi += sv[i][1];
    }
    SGi = rows_total64(SGi);
    SGQi = rows_total64(SGQi);
    const int bn = wave < CSq ? 0 : 1, c = (wave % CSq) * 16 + (lane & 15);
    if (lane < 16) {
      const lbt_chain_bwd_b& Bb = bn == 0 ? p.b1 : p.bs;
      const double s = (double)qstate(Bb.qn).inv_m, gsc = (double)qstate(Bb.qng).inv_m, nn = (double)Bb.n;
      const double SG = (double)SGi, SGQ = (double)SGQi;
      const float m = Bb.ms[c], sig = Bb.ms[Cq + c];
      const Recip rc = recip(sig);
      sh.cst[bn][0][c] = m;
      sh.cst[bn][1][c] = sig;
      sh.cst[bn][2][c] = rc.rc;
      sh.cst[bn][3][c] = (float)(gsc * SG / nn);
      sh.cst[bn][4][c] = (float)(gsc * (s * SGQ - (double)m * SG) / (nn * (double)sig));
    }
  }
  const QState sn1 = qstate(p.b1.qn), sns = qstate(p.bs.qn), sg1 = qstate(p.b1.qng), sgs = qstate(p.bs.qng);
  __syncthreads();
  LBT_TS(1);

  // ---------------- phase 1: both pass-B chains -> LDS gradient-code images
  int ova = 0, ovb = 0;
  const int g0w = __builtin_amdgcn_readfirstlane(tid) & ~63;  // the wave's first thread
  int s1a[4] = {0, 0, 0, 0}, s2a[4] = {0, 0, 0, 0}, s1b[4] = {0, 0, 0, 0}, s2b[4] = {0, 0, 0, 0};
#pragma unroll
  for (int it = 0; it < kIt; ++it) {
    if (it * kBThreads >= NG1 + NGS) break;  // uniform
    const int g = tid + it * kBThreads;
    const bool r1 = g < NG1;  // wave-uniform
    const int gg = r1 ? g : g - NG1;
    const bool valid = r1 || gg < NGS;
    const int pix = gg / Cq4, hy = pix / Wq, x = pix - hy * Wq;
    const int y = r1 ? q0 - 1 + hy : q0 + hy;
    const bool in = valid && (unsigned)y < (unsigned)Hq;
    const bool own = in && (!r1 || hy >= 1);
    const int bn = r1 ? 0 : 1;
    const QState& so = r1 ? so1 : sos;
    const QState& sn = r1 ? sn1 : sns;
    const QState& sgq = r1 ? sg1 : sgs;
    const float4 mu4 = *reinterpret_cast<const float4*>(&sh.cst[bn][0][cqq]);
    const float4 sg4 = *reinterpret_cast<const float4*>(&sh.cst[bn][1][cqq]);
    const float4 rc4 = *reinterpret_cast<const float4*>(&sh.cst[bn][2][cqq]);
    const float4 mg4 = *reinterpret_cast<const float4*>(&sh.cst[bn][3][cqq]);
    const float4 mx4 = *reinterpret_cast<const float4*>(&sh.cst[bn][4][cqq]);
    const pf2 mu2[2] = {pk(mu4.x, mu4.y), pk(mu4.z, mu4.w)}, sg2[2] = {pk(sg4.x, sg4.y), pk(sg4.z, sg4.w)};
    const pf2 rc2[2] = {pk(rc4.x, rc4.y), pk(rc4.z, rc4.w)}, mg2[2] = {pk(mg4.x, mg4.y), pk(mg4.z, mg4.w)};
    const pf2 mx2[2] = {pk(mx4.x, mx4.y), pk(mx4.z, mx4.w)};
    const float T1 = ov_thr(own, so.L), T2 = ov_thr(own, so.Lh);
    int G[4], q[4], c[4];
    unpack4_i8(Gv[it], G);
    unpack4_i8(Qv[it], q);
    const pf2 u[2] = {pk(Uv[it].x, Uv[it].y), pk(Uv[it].z, Uv[it].w)};
    int o = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const pf2 x1 = pcvt(q[2 * h], q[2 * h + 1]) * sn.inv_m;
      const pf2 x2 = x1 - mu2[h];
      const pf2 xh = pdiv_nz(x2, sg2[h], rc2[h]);
      const pf2 gh = pcvt(G[2 * h], G[2 * h + 1]) * sgq.inv_m;
      const pf2 t1 = gh - mg2[h];
      const pf2 t2 = xh * mx2[h];
      const pf2 dx = pdiv_nz(t1 - t2, sg2[h], rc2[h]);
      const pf2 xm = dx * so.m;
      ov_count2(xm, T1, T2, o);
      const pf2 fl = qfloor2(so, xm, u[h]);
      c[2 * h] = in ? (int)fl.x : 0;  // outside the image: the conv's zero padding
      c[2 * h + 1] = in ? (int)fl.y : 0;
    }
    const int w = pack4_i8(c);
    // r1 from the wave's first group: a scalar, so the wave totals stay on the scalar unit
    const bool r1w = it * kBThreads + g0w < NG1;
    ova += r1w ? o : 0;
    ovb += r1w ? 0 : o;
    if (r1) {
      *reinterpret_cast<int*>(sh.g1 + pix * Cq + cqq) = w;
      if (own) {
        st_out(p.b1.gq + imgq + (uint32_t)((y * Wq + x) * Cq + cqq), w);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          s1a[k] += c[k];
          s2a[k] += c[k] * c[k];
        }
      }
    } else {
      if (valid) *reinterpret_cast<int*>(sh.gs + pix * Cq + cqq) = w;
      if (own) {
        st_out(p.bs.gq + imgq + (uint32_t)((y * Wq + x) * Cq + cqq), w);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          s1b[k] += c[k];
          s2b[k] += c[k] * c[k];
        }
      }
    }
  }
  __syncthreads();
  LBT_TS(2);

  // phase-3 operands, issued now (they land while the MFMAs run)
  float4 ymv[J], urg[NB][J], ung[NB][J];
  int Rv[NB][J], qnv[NB][J];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int pix = (tid + j * kBThreads) / C4;
    const uint32_t off = (uint32_t)(r0 * W * C + pix * C + cq);
    if (CF & kAYMask) ymv[j] = ld_f32x4(A.y_mask, img + off);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const lbt_bwd_branch& Bb = b == 0 ? A.b1 : A.b2;
      Rv[b][j] = ld_i8x4(Bb.R, img + off);
      qnv[b][j] = ld_i8x4(Bb.qn_codes, img + off);
      urg[b][j] = ld_f32x4(Bb.qrg.noise, off);
      ung[b][j] = ld_f32x4(Bb.qng.noise, off);
    }
  }

  // ---------------- phase 2: dx = dgrad(3x3/2)  // ---------------- phase 2: dx = dgrad(3x3/2) + dgrad(1x1/2) from the LDS images
#pragma unroll
  for (int pi = 0; pi < TH / 4; ++pi) {
    const int pr = wave + 8 * pi;
    const int mt = pr / NT, nt = pr - mt * NT;
    const int m = mt * 16 + r;
    const int ly = m / W, px = m - ly * W;
    v4i acc = v4i{0, 0, 0, 0}, acc2 = v4i{0, 0, 0, 0};
#pragma unroll
    for (int kk = 0; kk < kK1; ++kk) {
      const int s = kk * 4 + kg;  // (tap, 16-channel slice of Cq)
      const int tap = s / CSq, cs = s - tap * CSq;
      const int kh = tap / 3, kw = tap - kh * 3;
      // dx row r0 + ly reads gq row (r0 + ly - kh) / 2 = local row (ly - kh) / 2 + 1 when even
      const bool ok = s < 9 * CSq && ((ly - kh) & 1) == 0 && ((px - kw) & 1) == 0 && px >= kw;
      const int lr = ((ly - kh) >> 1) + 1, ox = (px - kw) >> 1;
      v4i a = *reinterpret_cast<const v4i*>(sh.g1 + (ok ? (lr * Wq + ox) * Cq + cs * 16 : 0));
      if (!ok) a = v4i{0, 0, 0, 0};
      acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, bf1[kk], acc, 0, 0, 0);
    }
    {
      const bool ok = kg < CSq && (ly & 1) == 0 && (px & 1) == 0;
      v4i a = *reinterpret_cast<const v4i*>(sh.gs + (ok ? ((ly >> 1) * Wq + (px >> 1)) * Cq + kg * 16 : 0));
      if (!ok) a = v4i{0, 0, 0, 0};
      acc2 = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, bfs, acc2, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float v = (float)acc[i] * scale1, add = (float)acc2[i] * scale2;
      sh.tile[(mt * 16 + 4 * kg + i) * (C + 4) + nt * 16 + r] = v + add;
    }
  }
  __syncthreads();
  LBT_TS(3);

  // ---------------- phase 3: pass A over the tile (conv_bwd_kernel's phase 3)
  int ov[2][2] = {{0, 0}, {0, 0}};  // [branch][qrg | qng]
  int acc3[NB][4][4];
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int k = 0; k < 4; ++k) acc3[b][s][k] = 0;
  pf2 gam2a[NB][2], bet2a[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int b = 0; b < NB; ++b) gam2a[b][h] = pk(gam[b][2 * h], gam[b][2 * h + 1]);
    bet2a[h] = pk(bet[2 * h], bet[2 * h + 1]);
  }
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int pix = (tid + j * kBThreads) / C4;
    const uint32_t off = (uint32_t)(r0 * W * C + pix * C + cq);
    const float4 t = *reinterpret_cast<const float4*>(sh.tile + pix * (C + 4) + cq);
    pf2 g[2] = {pk(t.x, t.y), pk(t.z, t.w)};
    int R1[4];
    unpack4_i8(Rv[0][j], R1);
    if (CF & kAYMask) {
      const float ym[4] = {ymv[j].x, ymv[j].y, ymv[j].z, ymv[j].w};
#pragma unroll
      for (int h = 0; h < 2; ++h)
        g[h] = pk(ym[2 * h] > 0.f ? g[h].x : 0.f, ym[2 * h + 1] > 0.f ? g[h].y : 0.f);
    } else if (CF & kAMaskR) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const pf2 xr = pcvt(R1[2 * h], R1[2 * h + 1]) * r_inv;
        const pf2 m1 = xr * gam2a[0][h];
        const pf2 yv = m1 + bet2a[h];
        g[h] = pk(yv.x > 0.f ? g[h].x : 0.f, yv.y > 0.f ? g[h].y : 0.f);
      }
    }
    if (CF & kAGmask) st_out4(A.gmask_out, (uint32_t)(img + off), make_float4(g[0].x, g[0].y, g[1].x, g[1].y));
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const lbt_bwd_branch& Bb = b == 0 ? A.b1 : A.b2;
      int R[4], qn[4], Gc[4];
      unpack4_i8(Rv[b][j], R);
      unpack4_i8(qnv[b][j], qn);
      const pf2 ur[2] = {pk(urg[b][j].x, urg[b][j].y), pk(urg[b][j].z, urg[b][j].w)};
      const pf2 un[2] = {pk(ung[b][j].x, ung[b][j].y), pk(ung[b][j].z, ung[b][j].w)};
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const pf2 xm = g[h] * qrg[b].m;
        ov_count2(xm, qrg[b].L, qrg[b].Lh, ov[b][0]);
        const pf2 f1 = qfloor2(qrg[b], xm, ur[h]);  // G2 codes
        const pf2 gh = f1 * qrg[b].inv_m;
        const pf2 d = gh * gam2a[b][h];
        const pf2 dm = d * qng[b].m;
        ov_count2(dm, qng[b].L, qng[b].Lh, ov[b][1]);
        const pf2 f2c = qfloor2(qng[b], dm, un[h]);  // Gc codes
        const int G2[2] = {(int)f1.x, (int)f1.y};
        Gc[2 * h] = (int)f2c.x;
        Gc[2 * h + 1] = (int)f2c.y;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int k = 2 * h + i;
          acc3[b][0][k] += G2[i] * R[k];
          acc3[b][1][k] += G2[i];
          acc3[b][2][k] += Gc[k];
          acc3[b][3][k] += Gc[k] * qn[k];
        }
      }
      st_out(Bb.gout + img + off, pack4_i8(Gc));
    }
  }

  // ---------------- channel sums and counters (conv_bwd_kernel's publish, plus a second gq sum set)
  {
    const bool own = (lane & 15) < C4;
    int* part = sh.part[wave] + cq + (lane >> 4);
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int t = chan_scatter4(acc3[b][s], C4);
        if (own) part[(b * 4 + s) * C] = t;
      }
    const bool ownq = (lane & 15) < Cq4;
    int* pq = sh.part[wave] + NB * 4 * C + cqq + (lane >> 4);
    const int t1 = chan_scatter4(s1a, Cq4), t2 = chan_scatter4(s2a, Cq4);
    const int t3 = chan_scatter4(s1b, Cq4), t4 = chan_scatter4(s2b, Cq4);
    if (ownq) {
      pq[0] = t1;
      pq[Cq] = t2;
      pq[2 * Cq] = t3;
      pq[3 * Cq] = t4;
    }
  }
  constexpr int NQ = 2 + 2 * NB;  // [qo1 | qos | qrg, qng of branch 1 | of branch 2]
  ov_stage_w(0, NQ, ova, sh.cnt);
  ov_stage_w(1, NQ, ovb, sh.cnt);
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    ov_stage_w(2 + 2 * b, NQ, ov[b][0], sh.cnt);
    ov_stage_w(3 + 2 * b, NQ, ov[b][1], sh.cnt);
  }
  __syncthreads();
  LBT_TS(4);
  counts_publish_nw<kBNW>(0, NQ, p.b1.qo, sh.cnt);
  counts_publish_nw<kBNW>(1, NQ, p.bs.qo, sh.cnt);
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const lbt_bwd_branch& Bb = b == 0 ? A.b1 : A.b2;
    counts_publish_nw<kBNW>(2 + 2 * b, NQ, Bb.qrg, sh.cnt);
    counts_publish_nw<kBNW>(3 + 2 * b, NQ, Bb.qng, sh.cnt);
  }
  // slot i of [NB*4C pass-A sums | 2Cq conv-1 gq sums | 2Cq shortcut gq sums]
  const int shard = shard_id();
  for (int i = tid; i < NB * 4 * C + 4 * Cq; i += kBThreads) {
    long long v = 0;
#pragma unroll
    for (int w = 0; w < kBNW; ++w) v += sh.part[w][i];
    if (!v) continue;
    int64_t* dst;
    if (i < NB * 4 * C) {
      const int b = i / (4 * C);
      dst = (b == 0 ? A.b1 : A.b2).sums + (int64_t)shard * 4 * C + (i - b * 4 * C);
    } else {
      const int k = i - NB * 4 * C;
      const lbt_chain_bwd_b& Bb = k < 2 * Cq ? p.b1 : p.bs;
      if (!Bb.gcolsum) continue;
      dst = Bb.gcolsum + (int64_t)shard * 2 * Cq + (k < 2 * Cq ? k : k - 2 * Cq);
    }
    LBT_GADD((unsigned long long*)dst, (unsigned long long)v);
  }
  LBT_TS(5);
}

}  // namespace

extern "C" int lbt_conv_bwd2_fused_i8(const lbt_conv_bwd2* q, void* stream) {
  if (!q) return LBT_EINVAL;
  const lbt_conv_desc &d1 = q->d1, &ds = q->ds;
  const int C = d1.Cin, Cq = d1.Cout;
  // the projection block's 3x3/2 SAME conv (pads: top / left 0, bottom / right 1) and 1x1/2 shortcut
  if (!desc_ok(d1) || !desc_ok(ds) || d1.KH != 3 || d1.KW != 3 || d1.SH != 2 || d1.SW != 2 || d1.PT != 0 ||
      d1.PL != 0 || ds.KH != 1 || ds.KW != 1 || ds.SH != 2 || ds.SW != 2 || ds.PT != 0 || ds.PL != 0 ||
      (C != 16 && C != 32) || Cq != 2 * C || d1.W * C != 512 || d1.H % 2 || d1.W % 2 || d1.Ho * 2 != d1.H ||
      d1.Wo * 2 != d1.W || d1.H % tile_rows(C / 16) || ds.N != d1.N || ds.H != d1.H || ds.W != d1.W || ds.Cin != C ||
      ds.Cout != Cq || ds.Ho != d1.Ho || ds.Wo != d1.Wo || (int64_t)d1.N * d1.H * 512 >= ((int64_t)1 << 29))
    return LBT_EINVAL;
  const int CS = C / 16;
  const int64_t inq = (int64_t)d1.Ho * d1.Wo * Cq;
  const lbt_chain_bwd_b* bb[2] = {&q->b1, &q->bs};
  for (int i = 0; i < 2; ++i) {
    const lbt_chain_bwd_b& b = *bb[i];
    if (!b.G || !b.qn_codes || !b.ms || !b.sums || !b.gq || b.dx || !noise_ok(b.qo) || b.C != Cq || b.rows != d1.N ||
        b.inner != inq)
      return LBT_EINVAL;
  }
  const lbt_chain_bwd_a& a = q->a;
  if (a.C != C || a.rows != d1.N || a.inner != (int64_t)d1.H * d1.W * C) return LBT_EINVAL;
  const int f = bwd_a_flags(a);
  if ((f & kAFused) != kAFused) return LBT_EINVAL;
  for (int br = 0; br < (a.has_b2 ? 2 : 1); ++br) {
    const lbt_bwd_branch& Bb = br ? a.b2 : a.b1;
    if (!noise_ok(Bb.qrg) || !noise_ok(Bb.qng) || !Bb.gb) return LBT_EINVAL;
  }
  if (q->ksd1 != 4 * ((9 * 2 * CS + 3) / 4) || q->ksds != 4 || !q->wd1 || !q->wds) return LBT_EINVAL;
  if (q->w4 && (q->qw1.bits > 4 || q->qws.bits > 4)) return LBT_EINVAL;
  if (q->b1.qo.bits > 8 || q->bs.qo.bits > 8) return LBT_EINVAL;  // int8 gq codes; int32 channel sums of q^2
  ConvBwd2Args p;
  p.b1 = q->b1; p.bs = q->bs; p.wd1 = q->wd1; p.wds = q->wds; p.qw1 = q->qw1; p.qws = q->qws; p.H = d1.H; p.a = a;
  const int64_t tiles = (int64_t)d1.N * (d1.H / tile_rows(CS));
  if (tiles > 0x7fffffff || (int64_t)d1.N * d1.H * d1.W * C >= ((int64_t)1 << 31)) return LBT_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int nb = a.has_b2 ? 2 : 1;
#define LBT_B2(CS_, CF_, NB_)                                                                              \
  if (CS == CS_ && f == (CF_) && nb == NB_) {                                                              \
    if (q->w4)                                                                                             \
      hipLaunchKernelGGL((conv_bwd2_kernel<CS_, CF_, NB_, true>), dim3((unsigned)tiles), dim3(kBThreads), 0, st, p); \
    else                                                                                                   \
      hipLaunchKernelGGL((conv_bwd2_kernel<CS_, CF_, NB_, false>), dim3((unsigned)tiles), dim3(kBThreads), 0, st, p); \
    return (int)hipGetLastError();                                                                         \
  }
  // the consumer is an identity block's end chain (mask from y, masked gradient stored) or the
  // stem's (y mask only)
  LBT_B2(1, kAFused | kAYMask | kAGmask, 1)
  LBT_B2(2, kAFused | kAYMask | kAGmask, 1)
  LBT_B2(1, kAFused | kAYMask, 1)
  LBT_B2(2, kAFused | kAYMask, 1)
#undef LBT_B2
  return LBT_EINVAL;
}
