// conv_fused_fwd.h -- the fused conv forward kernel templates (conv_fused.h's scaffold), instantiated by
// conv_fused_fwd.hip (training mode: batch statistics) and conv_fused_infer.hip (INF: testing mode).
#pragma once
#include "conv_fused.h"

namespace lbt {
// The testing-mode launchers (conv_fused_infer.hip) behind lbt_conv_fwd_fused_i8 / lbt_conv_fwd2_fused_i8:
// every normalising branch of q->c has nrm.frozen set.
int conv_fwd_fused_infer(const lbt_conv_fwd* q, hipStream_t st);
int conv_fwd2_fused_infer(const lbt_conv_fwd2* q, hipStream_t st);
}  // namespace lbt

// ============================================================================ fused conv forward
// lbt_conv_fwd_fused_i8: the BN element chain that produces a stride-1 3x3 conv's input (bn.hip
// chain_fwd_kernel's arithmetic) runs as the conv's operand staging. A workgroup owns TH image
// rows: phase 1 evaluates the chain over the rows plus a one-pixel halo into an LDS image of the
// conv's input codes (owned pixels also store R codes / y / X codes and count overflows), phase 2
// runs the MFMAs from LDS into an fp32 LDS tile, phase 3 quantises the tile for the next BN (one
// channel quad per thread) and adds its channel sums.
// INF (testing mode, every branch frozen): mu / sigma are the running averages (bn_moments' frozen
// branch: sigma = sqrtf(run_var + eps)), read straight into the LDS cst slots -- no shard sums, no double
// arithmetic, no ms / running-average write; no overflow counting and no channel sums (the next BN is
// frozen too); the R-code and X-code stores, which only the backward reads, happen where a pointer is given.
namespace {

struct ConvFwdArgs {
  lbt_chain_fwd c;
  const int8_t* wf;
  const int32_t* wcolsum;
  lbt_qdesc qw;
  int H;
  int8_t* yq;
  lbt_qdesc qout;
  int64_t* ychsum;
};

template <int C, int TH, int WB, bool INF = false>
struct FwdShared {
  int8_t w[WB];                               // the forward weight image (WImg)
  int8_t x[(TH + 2) * (512 / C + 2) * C];   // the conv's input codes, halo image (q - 128)
  float tile[TH * (512 / C) * (C + 4)];      // conv outputs [TH*W][C+4]
  float cst[2][2][C];                          // per branch: mu, sigma
  int part[INF ? 1 : kBNW][2 * C];             // per wave: S1, S2 of the output codes (INF: unused)
  int cnt[INF ? 1 : kBNW * 2 * 4];             // counters: R (2 branches), X, output (INF: unused)
};

// waves per SIMD asked of the register allocator: the two-branch 2-row W4 tile of 32 channels keeps the 6
// it has always had (80 VGPRs: three workgroups per CU) -- at 4 the scalar overflow counters leave it 82
__host__ __device__ constexpr int fwd_waves(int CS, int NB, bool W4, int TH, bool INF) {
  return (CS == 4 && TH >= 4) ? 2 : (CS == 2 && NB == 2 && W4 && TH == 2 && !INF) ? 6 : 4;
}
template <int CS, int NB, int F, bool W4, int TH = tile_rows(CS), bool INF = false>
__global__ __launch_bounds__(kBThreads, fwd_waves(CS, NB, W4, TH, INF)) void conv_fwd_fused_kernel(ConvFwdArgs p) {
  using T = FusedTile<CS, TH>;
  constexpr int C = T::C, C4 = T::C4, NT = T::NT, W = T::W, Wp = T::Wp, kMaxKS = T::kMaxKS;
  constexpr int kBIt = T::kBIt, NQ = T::NQ, J = T::J, NPR = T::NPR;
  using WI = WImg<C, 4 * kMaxKS, W4>;
  __shared__ __attribute__((aligned(16))) FwdShared<C, TH, WI::kBytes, INF> sh;
  LBT_TS(0);
  const lbt_chain_fwd& a = p.c;
  const int H = p.H;
  const uint32_t bid = blockIdx.x;
  const int tpi = H / TH;
  const int n = (int)(bid / (uint32_t)tpi), row0 = (int)(bid - (uint32_t)n * tpi) * TH;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, kg = lane >> 4;
  const int cq = (tid % C4) * 4;
  const int64_t img = (int64_t)n * H * W * C;
  constexpr bool RES = (F & kFRes) != 0, YST = (F & kFY) != 0;

  // ---------------- the moments' shard sums first (they gate the first barrier), then the loads that
  // do not depend on the moments
  // waves w < NB*C/16 each own 16 (branch, channel) pairs: lane l reads pair w*16 + (l & 15) of
  // shards 8*(l >> 4) .. +7 (each load instruction: 4 shards x 16 consecutive channels)
  static_assert(LBT_NSHARD == 32 && kBThreads == 512 && (NB * C) % 16 == 0 && NB * C / 16 <= kBNW,
                "moments layout");
  constexpr int kSW = NB * C / 16;  // statistics waves
  long long sv[8][2];
  float rmean = 0.f, rvar = 0.f;  // INF: the running averages of (branch, channel) pair tid
  if constexpr (INF) {
    if (tid < NB * C) {
      const lbt_bn_norm& nb = tid < C ? a.b1.nrm : a.b2.nrm;
      rmean = nb.run_mean[tid % C];
      rvar = nb.run_var[tid % C];
    }
  } else if (wave < kSW) {  // uniform per wave
    const int bc = wave * 16 + (lane & 15), b = bc / C, c = bc - b * C;
    const int64_t* cs = (b == 0 ? a.b1 : a.b2).nrm.chsum + (int64_t)(8 * (lane >> 4)) * 2 * C + c;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      sv[i][0] = cs[(int64_t)i * 2 * C];
      sv[i][1] = cs[(int64_t)i * 2 * C + C];
    }
  }
  // the chain's operands over the halo rows ylo .. yhi inside the image, whole rows of W pixels (as
  // conv_bwd_kernel; the padding cells: halo_pad_fill)
  const int ylo = row0 > 0 ? row0 - 1 : 0, yhi = row0 + TH < H ? row0 + TH : H - 1;
  const int ngrp = (yhi - ylo + 1) * W * C4;  // a multiple of 128: whole waves
  int qv[NB][kBIt];
  float4 rv[kBIt], nrv[NB][kBIt], nov[kBIt];
#pragma unroll
  for (int it = 0; it < kBIt; ++it) {
    const int g = tid + it * kBThreads;
    const uint32_t off = g < ngrp ? (uint32_t)((ylo * W + g / C4) * C + cq) : 0u;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const lbt_chain_branch& Bb = b == 0 ? a.b1 : a.b2;
      qv[b][it] = ld_i8x4(Bb.nrm.q, img + off);
      nrv[b][it] = ld_f32x4(Bb.qr.noise, off);
    }
    if constexpr (RES) rv[it] = ld_f32x4(a.res, img + off);
    nov[it] = ld_f32x4(a.qo1.noise, off);
  }
  // the B operands (the forward weight image, for LDS: WImg): loaded in this first load wave, stored
  // to LDS at the end of phase 1
  v4i wimg[WI::kIt];
  WI::load(p.wf, wimg);
  const int bcol = (wave % NT) * 16 + r;
  const int corr = 128 * p.wcolsum[bcol];  // the unsigned-9-bit offset encoding undone: + 128 * sum_k W[k][col]
  float gam[NB][4], bet[NB][4];
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      gam[b][k] = (b == 0 ? a.b1 : a.b2).gb[cq + k];
      bet[b][k] = (b == 0 ? a.b1 : a.b2).gb[C + cq + k];
    }
  QState qr[2];
  float sn[2];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    qr[b] = qstate((b == 0 ? a.b1 : a.b2).qr);
    sn[b] = qscale((b == 0 ? a.b1 : a.b2).nrm.qn);
  }
  const QState so1 = qstate(a.qo1), sq = qstate(p.qout);
  const float scale = ldexpf(1.0f, -(frac_exp(a.qo1) + frac_exp(p.qw)));

  // ---------------- Normalization_q moments (bn.hip bn_moments) from the shard sums loaded above: each
  // statistics wave adds its 8 shards per lane, then its four lane rows; lanes < 16 finish a pair.
  // (Was: threads c < C loading all 2 x 32 shards each -- 64 dependent-issue loads in one wave on
  // the launch's critical path.)
  if constexpr (INF) {  // testing mode: bn_moments' frozen branch, nothing written back
    if (tid < NB * C) {
      const float eps = (tid < C ? a.b1.nrm : a.b2.nrm).eps;
      sh.cst[tid / C][0][tid % C] = rmean;
      sh.cst[tid / C][1][tid % C] = sqrtf(rvar + eps);
    }
  } else if (wave < kSW) {
    long long S1 = 0, S2 = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      S1 += sv[i][0];
      S2 += sv[i][1];
    }
    S1 = rows_total64(S1);
    S2 = rows_total64(S2);
    const int bc = wave * 16 + (lane & 15), b = bc / C, c = bc - b * C;
    if (lane < 16) {
    const lbt_bn_norm& nb = b == 0 ? a.b1.nrm : a.b2.nrm;
    const double s = ldexp(1.0, -frac_exp(nb.qn));
    const double mean_d = (double)S1 * s / (double)nb.n;
    const double var_d = (double)S2 * (s * s) / (double)nb.n - mean_d * mean_d;
    const float m = (float)mean_d, vv = (float)var_d;
    const float sigma = sqrtf(vv + nb.eps);
    sh.cst[b][0][c] = m;
    sh.cst[b][1][c] = sigma;
    if (bid == 0) {  // one writer: ms for the backward, the running averages (:601-612)
      if (nb.ms) { nb.ms[c] = m; nb.ms[C + c] = sigma; }
      if (nb.run_mean) {
        nb.run_mean[c] = nb.momentum * nb.run_mean[c] + nb.one_minus_momentum * m;
        nb.run_var[c] = nb.momentum * nb.run_var[c] + nb.one_minus_momentum * vv;
      }
    }
    }
  }
  __syncthreads();
  LBT_TS(1);
  float pm[NB][4];
  Recip ps[NB][4];
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      pm[b][k] = sh.cst[b][0][cq + k];
      ps[b][k] = recip(sh.cst[b][1][cq + k]);
    }
  pf2 pm2[NB][2], psy2[NB][2], psr2[NB][2], gam2[NB][2], bet2[NB][2];
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      pm2[b][h] = pk(pm[b][2 * h], pm[b][2 * h + 1]);
      psy2[b][h] = pk(ps[b][2 * h].y, ps[b][2 * h + 1].y);
      psr2[b][h] = pk(ps[b][2 * h].rc, ps[b][2 * h + 1].rc);
      gam2[b][h] = pk(gam[b][2 * h], gam[b][2 * h + 1]);
      bet2[b][h] = pk(bet[b][2 * h], bet[b][2 * h + 1]);
    }

  // ---------------- phase 1: the chain over the rows + halo -> LDS input codes
  // the wave index as a scalar where counters are compiled: the wave-uniform loop exits and halo tests are
  // then scalar branches and selects, and the overflow totals (ov_count2) never pass through a VGPR
  int wu = wave;
  if constexpr (!INF) wu = __builtin_amdgcn_readfirstlane(wave);
  int ovr[2] = {0, 0}, ovx = 0;
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
    const uint32_t e = (uint32_t)((y * W + x) * C + cq);
    pf2 v[2];  // the channel quad as two packed pairs
    float T1[2], T2[2];
    if constexpr (!INF) {
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        T1[b] = ov_thr(nanw, qr[b].L);
        T2[b] = ov_thr(nanw, qr[b].Lh);
      }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const lbt_chain_branch& Bb = b == 0 ? a.b1 : a.b2;
      int q[4];
      unpack4_i8(qv[b][it], q);
      const pf2 u[2] = {pk(nrv[b][it].x, nrv[b][it].y), pk(nrv[b][it].z, nrv[b][it].w)};
      pf2 fl[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const pf2 x1 = pcvt(q[2 * h], q[2 * h + 1]) * sn[b];
        const pf2 x2 = x1 - pm2[b][h];
        const pf2 t = pdiv_nz(x2, psy2[b][h], psr2[b][h]);
        const pf2 xm = t * qr[b].m;
        if constexpr (!INF) ov_count2(xm, T1[b], T2[b], ovr[b]);
        fl[h] = qfloor2(qr[b], xm, u[h]);  // the R codes
        const pf2 xr = fl[h] * qr[b].inv_m;
        const pf2 m1 = xr * gam2[b][h];
        const pf2 tt = m1 + bet2[b][h];
        v[h] = b ? v[h] + tt : tt;
      }
      if (own && (!INF || Bb.rout)) st_out(Bb.rout + img + e, pack4f(fl[0], fl[1]));
    }
    if constexpr (RES) {
      v[0] = v[0] + pk(rv[it].x, rv[it].y);
      v[1] = v[1] + pk(rv[it].z, rv[it].w);
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) v[h] = pk(v[h].x > 0.f ? v[h].x : 0.f, v[h].y > 0.f ? v[h].y : 0.f);
    if (YST && own) st_out4(a.y, (uint32_t)(img + e), make_float4(v[0].x, v[0].y, v[1].x, v[1].y));
    const pf2 uo[2] = {pk(nov[it].x, nov[it].y), pk(nov[it].z, nov[it].w)};
    const float X1 = ov_thr(nanw, so1.L), X2 = ov_thr(nanw, so1.Lh);
    int co[4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      // v >= 0 after the ReLU (NaN -> 0): the lower clip and x < -L cannot hold, the codes are >= 0
      const pf2 xm = v[h] * so1.m;
      if constexpr (!INF) ov_count2_pos(xm, X1, X2, ovx);
      const pf2 w = xm + uo[h];
      co[2 * h] = floor_i(fminf(w.x, so1.Lm1));
      co[2 * h + 1] = floor_i(fminf(w.y, so1.Lm1));
    }
    // LBT_OUT_U8OFF: code - 128 (= code ^ 0x80 for codes in [0, 255])
    const int cw = pack4_i8(co) ^ (int)0x80808080;
    *reinterpret_cast<int*>(sh.x + pix * C + cq) = cw;
    if (own && (!INF || a.o1)) st_out((int8_t*)a.o1 + img + e, cw);
  }
  halo_pad_fill<C, TH>(sh.x, row0, H, (int)0x80808080);  // outside the image: the offset code of 0
  WI::store(sh.w, wimg);
  __syncthreads();
  LBT_TS(2);
  // phase-3 noise (the output quantiser), issued under the MFMAs
  float4 u3[J];  // J channel quads per thread: NQ <= J * kBThreads (the idle threads load the first quad)
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int q3 = tid + j * kBThreads;
    u3[j] = ld_f32x4(p.qout.noise, (uint32_t)(row0 * W * C + ((q3 < NQ ? q3 : 0) / C4) * C + cq));
  }

  // ---------------- phase 2: the conv from the LDS image (pair = wave + 8 pi)
#pragma unroll
  for (int pi = 0; pi < (NPR + 7) / 8; ++pi) {
    const int pr = wave + 8 * pi;
    if (NPR % 8 && pr >= NPR) break;  // uniform per wave
    const int mt = pr / NT, nt = pr - mt * NT;
    const int m = mt * 16 + r;
    const int ly = m / W, px = m - ly * W;
    const int8_t* base = sh.x + (ly * Wp + px) * C;
    v4i acc = v4i{0, 0, 0, 0};
#pragma unroll
    for (int kk = 0; kk < kMaxKS; ++kk) {
      const int s = kk * 4 + kg;
      const int tap = s / CS, cs = s - tap * CS;
      const int kh = tap / 3, kw = tap - kh * 3;
      v4i av = *reinterpret_cast<const v4i*>(base + (kh * Wp + kw) * C + cs * 16);
      if (s >= 9 * CS) av = v4i{0, 0, 0, 0};  // k padding (its weights are zero too)
      acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, WI::frag(sh.w, nt * 16 + r, s), acc, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
      sh.tile[(mt * 16 + 4 * kg + i) * (C + 4) + nt * 16 + r] = (float)(acc[i] + corr) * scale;
  }
  __syncthreads();
  LBT_TS(3);

  // ---------------- phase 3: the next BN's input quantiser + its channel sums
  int ovq = 0;
  int s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < J; ++j) {
    if (NQ % kBThreads && (INF ? tid : wu * 64) + j * kBThreads >= NQ) break;  // uniform per wave (NQ % 64 == 0)
    const int pix3 = (tid + j * kBThreads) / C4;
    const float4 t = *reinterpret_cast<const float4*>(sh.tile + pix3 * (C + 4) + cq);
    const pf2 tv[2] = {pk(t.x, t.y), pk(t.z, t.w)};
    const pf2 u[2] = {pk(u3[j].x, u3[j].y), pk(u3[j].z, u3[j].w)};
    pf2 fl[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const pf2 xm = tv[h] * sq.m;
      if constexpr (!INF) ov_count2(xm, sq.L, sq.Lh, ovq);
      fl[h] = qfloor2(sq, xm, u[h]);
    }
    const int c[4] = {(int)fl[0].x, (int)fl[0].y, (int)fl[1].x, (int)fl[1].y};
    if constexpr (!INF) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        s1[k] += c[k];
        s2[k] += c[k] * c[k];
      }
    }
    st_out(p.yq + img + (uint32_t)(row0 * W * C + pix3 * C + cq), pack4_i8(c));
  }
  if constexpr (!INF) {  // (INF: no channel sums -- the next BN is frozen too -- and no counters)
    {
      const int t1 = chan_scatter4(s1, C4), t2 = chan_scatter4(s2, C4);  // row lane >> 4: channel cq + row
      if ((lane & 15) < C4) {
        sh.part[wave][cq + (lane >> 4)] = t1;
        sh.part[wave][C + cq + (lane >> 4)] = t2;
      }
    }
    // slots [qr of branch 1 | qr of branch 2 | qo1 | qout]
#pragma unroll
    for (int b = 0; b < NB; ++b) ov_stage_w(b, 4, ovr[b], sh.cnt);
    ov_stage_w(2, 4, ovx, sh.cnt);
    ov_stage_w(3, 4, ovq, sh.cnt);
    __syncthreads();
    LBT_TS(4);
#pragma unroll
    for (int b = 0; b < NB; ++b) counts_publish_nw<kBNW>(b, 4, (b == 0 ? a.b1 : a.b2).qr, sh.cnt);
    counts_publish_nw<kBNW>(2, 4, a.qo1, sh.cnt);
    counts_publish_nw<kBNW>(3, 4, p.qout, sh.cnt);
    if (p.ychsum && tid < 2 * C) {
      long long t = 0;
#pragma unroll
      for (int w = 0; w < kBNW; ++w) t += sh.part[w][tid];
      if (t) LBT_GADD((unsigned long long*)&p.ychsum[(int64_t)shard_id() * 2 * C + tid], (unsigned long long)t);
    }
  }
  LBT_TS(5);
}

// ---- lbt_conv_fwd2_fused_i8: a stage transition's forward in ONE launch -- the last identity block's
// end chain (bn2 + residual + ReLU, its R codes and fp32 y, and BOTH of the projection block's input
// quantisers: the 3x3/2 conv's and the 1x1/2 shortcut's) evaluated into LDS code images, the two
// strided convs from LDS, and both BNs' input quantisers + channel sums over the two conv tiles.
// Bit-identical to lbt_bn_chain_fwd + lbt_conv_fwd_pair_i8. A workgroup owns TH2 output rows, i.e.
// input rows 2 oy0 .. 2 oy0 + 2 TH2 - 1 (+ the row below: the 3x3/2 SAME padding is bottom / right).
constexpr int kTH2 = 4;  // output rows per workgroup (2 x 4 m-tiles: one (m, n) pair per wave)

struct ConvFwd2Args {
  lbt_chain_fwd c;
  const int8_t* wf1;
  const int8_t* wfs;
  const int32_t* wcolsum1;
  const int32_t* wcolsums;
  lbt_qdesc qw1, qws;
  int H;  // input rows
  int8_t* yq1;
  int8_t* yqs;
  lbt_qdesc qout1, qouts;
  int64_t* ychsum1;
  int64_t* ychsums;
};

template <int C, bool INF = false>
struct Fwd2Shared {
  int8_t xa[(2 * kTH2 + 1) * 512];          // the 3x3/2 conv's input codes (q - 128), rows 2oy0 .. 2oy0+2TH2
  int8_t xs[kTH2 * 256];                     // the shortcut's, even rows / columns only ([TH2][W/2][C])
  float tile[2][kTH2 * (256 / C) * (2 * C + 4)];  // the two conv outputs [pixel][Cq + 4]
  float cst[2][C];                           // bn2: mu, sigma
  int part[INF ? 1 : kBNW][2 * 2 * 2 * C];   // per wave: S1, S2 of both output code sets (2Cq each; INF: unused)
  int cnt[INF ? 1 : kBNW * 2 * 5];           // counters: qr, qo1, qo2, qout1, qouts (INF: unused)
};

// INF: testing mode, as conv_fwd_fused_kernel's.
template <int CS, bool W4, bool INF = false>
__global__ __launch_bounds__(kBThreads, CS == 1 ? 4 : 2) void conv_fwd2_kernel(ConvFwd2Args p) {
  using T = FusedTile<CS, 2 * kTH2>;  // (2 TH2 input rows)
  constexpr int C = T::C, C4 = T::C4, W = T::W, Cq = 2 * C, Cq4 = Cq / 4, Wq = W / 2, NTq = Cq / 16;
  constexpr int kK1 = T::kMaxKS;
  constexpr int NG = (2 * kTH2 + 1) * W * C4;  // chain groups (rows 2oy0 .. 2oy0 + 2TH2)
  constexpr int kIt = (NG + kBThreads - 1) / kBThreads;
  static_assert(kTH2 * Wq * Cq == 2 * 1024 && C / 16 <= kBNW, "layout");
  __shared__ __attribute__((aligned(16))) Fwd2Shared<C, INF> sh;
  LBT_TS(0);
  const lbt_chain_fwd& a = p.c;
  const int H = p.H, Hq = H / 2;
  const uint32_t bid = blockIdx.x;
  const int tpi = Hq / kTH2;
  const int n = (int)(bid / (uint32_t)tpi), oy0 = (int)(bid - (uint32_t)n * tpi) * kTH2, y0 = 2 * oy0;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, kg = lane >> 4;
  const int cq = (tid % C4) * 4, cqq = (tid % Cq4) * 4;
  const int64_t img = (int64_t)n * H * W * C, imgq = (int64_t)n * Hq * Wq * Cq;

  // ---------------- bn2's moment shard sums first (waves w < C / 16), then every other load
  constexpr int kSW = C / 16;
  long long sv[8][2];
  float rmean = 0.f, rvar = 0.f;  // INF: channel tid's running averages
  if constexpr (INF) {
    if (tid < C) {
      rmean = a.b1.nrm.run_mean[tid];
      rvar = a.b1.nrm.run_var[tid];
    }
  } else if (wave < kSW) {
    const int c = wave * 16 + (lane & 15);
    const int64_t* cs = a.b1.nrm.chsum + (int64_t)(8 * (lane >> 4)) * 2 * C + c;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      sv[i][0] = cs[(int64_t)i * 2 * C];
      sv[i][1] = cs[(int64_t)i * 2 * C + C];
    }
  }
  int qv[kIt];
  float4 rv[kIt], nrv[kIt], no1[kIt], no2[kIt];
#pragma unroll
  for (int it = 0; it < kIt; ++it) {
    const int g = tid + it * kBThreads;
    const int pix = g / C4, hy = pix / W, x = pix - hy * W;
    const int y = y0 + hy;
    const bool in = g < NG && y < H;
    const uint32_t off = in ? (uint32_t)((y * W + x) * C + cq) : 0u;
    qv[it] = ld_i8x4(a.b1.nrm.q, img + off);
    nrv[it] = ld_f32x4(a.b1.qr.noise, off);
    rv[it] = ld_f32x4(a.res, img + off);
    no1[it] = ld_f32x4(a.qo1.noise, off);
    no2[it] = ld_f32x4(a.qo2.noise, off);
  }
  // the two convs' B operands (forward weight images) of this wave's n-tile; one (m, n) pair per wave
  const int mt = wave / NTq, nt = wave - mt * NTq;
  const int bcol = nt * 16 + r;
  v4i bf1[kK1], bfs;
#pragma unroll
  for (int kk = 0; kk < kK1; ++kk) {
    if constexpr (W4)
      bf1[kk] = unpack_i4x16(*reinterpret_cast<const v2i*>(p.wf1 + ((int64_t)bcol * (4 * kK1) + kk * 4 + kg) * 8));
    else
      bf1[kk] = *reinterpret_cast<const v4i*>(p.wf1 + ((int64_t)bcol * (4 * kK1) + kk * 4 + kg) * 16);
  }
  if constexpr (W4)
    bfs = unpack_i4x16(*reinterpret_cast<const v2i*>(p.wfs + ((int64_t)bcol * 4 + kg) * 8));
  else
    bfs = *reinterpret_cast<const v4i*>(p.wfs + ((int64_t)bcol * 4 + kg) * 16);
  const int corr1 = 128 * p.wcolsum1[bcol], corr2 = 128 * p.wcolsums[bcol];
  float gam[4], bet[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    gam[k] = a.b1.gb[cq + k];
    bet[k] = a.b1.gb[C + cq + k];
  }
  const QState qr = qstate(a.b1.qr), so1 = qstate(a.qo1), so2 = qstate(a.qo2);
  const QState sq1 = qstate(p.qout1), sqs = qstate(p.qouts);
  const float sn = qscale(a.b1.nrm.qn);
  const float scale1 = ldexpf(1.0f, -(frac_exp(a.qo1) + frac_exp(p.qw1)));
  const float scale2 = ldexpf(1.0f, -(frac_exp(a.qo2) + frac_exp(p.qws)));

  // ---------------- Normalization_q moments (conv_fwd_fused_kernel's arithmetic)
  if constexpr (INF) {
    if (tid < C) {
      sh.cst[0][tid] = rmean;
      sh.cst[1][tid] = sqrtf(rvar + a.b1.nrm.eps);
    }
  } else if (wave < kSW) {
    long long S1 = 0, S2 = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      S1 += sv[i][0];
      S2 += sv[i][1];
    }
    S1 = rows_total64(S1);
    S2 = rows_total64(S2);
    const int c = wave * 16 + (lane & 15);
    if (lane < 16) {
      const lbt_bn_norm& nb = a.b1.nrm;
      const double s = ldexp(1.0, -frac_exp(nb.qn));
      const double mean_d = (double)S1 * s / (double)nb.n;
      const double var_d = (double)S2 * (s * s) / (double)nb.n - mean_d * mean_d;
      const float m = (float)mean_d, vv = (float)var_d;
      const float sigma = sqrtf(vv + nb.eps);
      sh.cst[0][c] = m;
      sh.cst[1][c] = sigma;
      if (bid == 0) {  // one writer: ms for the backward, the running averages (:601-612)
        if (nb.ms) { nb.ms[c] = m; nb.ms[C + c] = sigma; }
        if (nb.run_mean) {
          nb.run_mean[c] = nb.momentum * nb.run_mean[c] + nb.one_minus_momentum * m;
          nb.run_var[c] = nb.momentum * nb.run_var[c] + nb.one_minus_momentum * vv;
        }
      }
    }
  }
  __syncthreads();
  LBT_TS(1);
  pf2 pm2[2], psy2[2], psr2[2], gam2[2], bet2[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const Recip r0 = recip(sh.cst[1][cq + 2 * h]), r1 = recip(sh.cst[1][cq + 2 * h + 1]);
    pm2[h] = pk(sh.cst[0][cq + 2 * h], sh.cst[0][cq + 2 * h + 1]);
    psy2[h] = pk(r0.y, r1.y);
    psr2[h] = pk(r0.rc, r1.rc);
    gam2[h] = pk(gam[2 * h], gam[2 * h + 1]);
    bet2[h] = pk(bet[2 * h], bet[2 * h + 1]);
  }

  // ---------------- phase 1: the chain over the input rows -> the two LDS code images
  int ovr = 0, ovx = 0, ovs = 0;
#pragma unroll
  for (int it = 0; it < kIt; ++it) {
    if (it * kBThreads >= NG) break;  // uniform
    const int g = tid + it * kBThreads;
    const int pix = g / C4, hy = pix / W, x = pix - hy * W;
    const int y = y0 + hy;
    const bool valid = g < NG;
    const bool in = valid && y < H;
    const bool own = in && hy < 2 * kTH2;
    const uint32_t e = (uint32_t)((y * W + x) * C + cq);
    int q[4];
    unpack4_i8(qv[it], q);
    const pf2 u[2] = {pk(nrv[it].x, nrv[it].y), pk(nrv[it].z, nrv[it].w)};
    const float T1 = ov_thr(own, qr.L), T2 = ov_thr(own, qr.Lh);
    pf2 fl[2], v[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const pf2 x1 = pcvt(q[2 * h], q[2 * h + 1]) * sn;
      const pf2 x2 = x1 - pm2[h];
      const pf2 t = pdiv_nz(x2, psy2[h], psr2[h]);
      const pf2 xm = t * qr.m;
      if constexpr (!INF) ov_count2(xm, T1, T2, ovr);
      fl[h] = qfloor2(qr, xm, u[h]);  // the R codes
      const pf2 xr = fl[h] * qr.inv_m;
      const pf2 m1 = xr * gam2[h];
      v[h] = m1 + bet2[h];
    }
    if (own && (!INF || a.b1.rout)) st_out(a.b1.rout + img + e, pack4f(fl[0], fl[1]));
    v[0] = v[0] + pk(rv[it].x, rv[it].y);
    v[1] = v[1] + pk(rv[it].z, rv[it].w);
#pragma unroll
    for (int h = 0; h < 2; ++h) v[h] = pk(v[h].x > 0.f ? v[h].x : 0.f, v[h].y > 0.f ? v[h].y : 0.f);
    if (own) st_out4(a.y, (uint32_t)(img + e), make_float4(v[0].x, v[0].y, v[1].x, v[1].y));
    const pf2 u1[2] = {pk(no1[it].x, no1[it].y), pk(no1[it].z, no1[it].w)};
    const pf2 u2[2] = {pk(no2[it].x, no2[it].y), pk(no2[it].z, no2[it].w)};
    const float X1 = ov_thr(own, so1.L), X2 = ov_thr(own, so1.Lh);
    const float Z1 = ov_thr(own, so2.L), Z2 = ov_thr(own, so2.Lh);
    int c1[4], c2[4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      // v >= 0 after the ReLU: only the upper clip can act, the codes are >= 0
      const pf2 xm = v[h] * so1.m;
      if constexpr (!INF) ov_count2_pos(xm, X1, X2, ovx);
      const pf2 w1 = xm + u1[h];
      c1[2 * h] = floor_i(fminf(w1.x, so1.Lm1));
      c1[2 * h + 1] = floor_i(fminf(w1.y, so1.Lm1));
      const pf2 zm = v[h] * so2.m;
      if constexpr (!INF) ov_count2_pos(zm, Z1, Z2, ovs);
      const pf2 w2 = zm + u2[h];
      c2[2 * h] = floor_i(fminf(w2.x, so2.Lm1));
      c2[2 * h + 1] = floor_i(fminf(w2.y, so2.Lm1));
    }
    // LBT_OUT_U8OFF (code ^ 0x80); below the image: the code of 0
    const int cw1 = in ? (pack4_i8(c1) ^ (int)0x80808080) : (int)0x80808080;
    const int cw2 = in ? (pack4_i8(c2) ^ (int)0x80808080) : (int)0x80808080;
    if (valid) *reinterpret_cast<int*>(sh.xa + pix * C + cq) = cw1;
    if (own && !(hy & 1) && !(x & 1)) *reinterpret_cast<int*>(sh.xs + ((hy >> 1) * Wq + (x >> 1)) * C + cq) = cw2;
    if constexpr (INF) {  // the X codes live in the LDS images; the backward's copies where asked for
      if (own && a.o1) st_out((int8_t*)a.o1 + img + e, cw1);
      if (own && a.o2) st_out((int8_t*)a.o2 + img + e, cw2);
    } else if (own) {
      st_out((int8_t*)a.o1 + img + e, cw1);
      st_out((int8_t*)a.o2 + img + e, cw2);
    }
  }
  __syncthreads();
  LBT_TS(2);
  // phase-3 noise of both output quantisers (one quad of each tile per thread: TH2*Wq*Cq/4 == 512)
  const uint32_t off3 = (uint32_t)(oy0 * Wq * Cq + (tid / Cq4) * Cq + cqq);
  const float4 un1 = ld_f32x4(p.qout1.noise, off3), uns = ld_f32x4(p.qouts.noise, off3);

  // ---------------- phase 2: both strided convs from LDS (output pixel (ly, px) reads input
  // (2 ly + kh, 2 px + kw); column W is the SAME padding: the code of 0)
  {
    const int m = mt * 16 + r;
    const int ly = m / Wq, px = m - ly * Wq;
    v4i acc = v4i{0, 0, 0, 0}, acc2 = v4i{0, 0, 0, 0};
#pragma unroll
    for (int kk = 0; kk < kK1; ++kk) {
      const int s = kk * 4 + kg;
      const int tap = s / CS, cs = s - tap * CS;
      const int kh = tap / 3, kw = tap - kh * 3;
      const int ix = 2 * px + kw;
      const bool okx = ix < W;
      v4i av = *reinterpret_cast<const v4i*>(sh.xa + (((2 * ly + kh) * W + (okx ? ix : 0)) * C + cs * 16));
      if (!okx) av = v4i{(int)0x80808080, (int)0x80808080, (int)0x80808080, (int)0x80808080};
      if (s >= 9 * CS) av = v4i{0, 0, 0, 0};  // k padding (its weights are zero too)
      acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, bf1[kk], acc, 0, 0, 0);
    }
    {
      v4i av = *reinterpret_cast<const v4i*>(sh.xs + ((ly * Wq + px) * C + (kg < CS ? kg : 0) * 16));
      if (kg >= CS) av = v4i{0, 0, 0, 0};
      acc2 = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, bfs, acc2, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = (mt * 16 + 4 * kg + i) * (Cq + 4) + nt * 16 + r;
      sh.tile[0][row] = (float)(acc[i] + corr1) * scale1;
      sh.tile[1][row] = (float)(acc2[i] + corr2) * scale2;
    }
  }
  __syncthreads();
  LBT_TS(3);

  // ---------------- phase 3: both BNs' input quantisers + channel sums
  int ovq[2] = {0, 0};
  int s1[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}}, s2[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
  {
    const int pix3 = tid / Cq4;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const QState& sq = b ? sqs : sq1;
      const float4 un = b ? uns : un1;
      const float4 t = *reinterpret_cast<const float4*>(sh.tile[b] + pix3 * (Cq + 4) + cqq);
      const pf2 tv[2] = {pk(t.x, t.y), pk(t.z, t.w)};
      const pf2 u[2] = {pk(un.x, un.y), pk(un.z, un.w)};
      pf2 fl[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const pf2 xm = tv[h] * sq.m;
        if constexpr (!INF) ov_count2(xm, sq.L, sq.Lh, ovq[b]);
        fl[h] = qfloor2(sq, xm, u[h]);
      }
      const int c[4] = {(int)fl[0].x, (int)fl[0].y, (int)fl[1].x, (int)fl[1].y};
      if constexpr (!INF) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          s1[b][k] += c[k];
          s2[b][k] += c[k] * c[k];
        }
      }
      st_out((b ? p.yqs : p.yq1) + imgq + off3, pack4_i8(c));
    }
  }
  if constexpr (!INF) {  // (INF: no channel sums, no counters)
    {
      const bool ownq = (lane & 15) < Cq4;
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int t1 = chan_scatter4(s1[b], Cq4), t2 = chan_scatter4(s2[b], Cq4);
        if (ownq) {
          sh.part[wave][b * 2 * Cq + cqq + (lane >> 4)] = t1;
          sh.part[wave][b * 2 * Cq + Cq + cqq + (lane >> 4)] = t2;
        }
      }
    }
    // slots [qr | qo1 | qo2 | qout1 | qouts]
    ov_stage_w(0, 5, ovr, sh.cnt);
    ov_stage_w(1, 5, ovx, sh.cnt);
    ov_stage_w(2, 5, ovs, sh.cnt);
    ov_stage_w(3, 5, ovq[0], sh.cnt);
    ov_stage_w(4, 5, ovq[1], sh.cnt);
    __syncthreads();
    LBT_TS(4);
    counts_publish_nw<kBNW>(0, 5, a.b1.qr, sh.cnt);
    counts_publish_nw<kBNW>(1, 5, a.qo1, sh.cnt);
    counts_publish_nw<kBNW>(2, 5, a.qo2, sh.cnt);
    counts_publish_nw<kBNW>(3, 5, p.qout1, sh.cnt);
    counts_publish_nw<kBNW>(4, 5, p.qouts, sh.cnt);
    if (tid < 4 * Cq) {
      long long t = 0;
#pragma unroll
      for (int w = 0; w < kBNW; ++w) t += sh.part[w][tid];
      int64_t* dst = tid < 2 * Cq ? p.ychsum1 : p.ychsums;
      if (t && dst) LBT_GADD((unsigned long long*)&dst[(int64_t)shard_id() * 2 * Cq + (tid % (2 * Cq))], (unsigned long long)t);
    }
  }
  LBT_TS(5);
}

}  // namespace
