// igemm_big.hip -- the wide implicit GEMMs of igemm.hip on 256-row tiles, and lbt_igemm_tuning.
// igemm_big_kernel: the same implicit GEMMs (no split-K, no parity classes) on 256-row x BN-column
// workgroup tiles of 8 waves (wave tile (256 / WM) x 64, WM x WN = 8, WN = BN / 64), with BOTH operands
// staged by LDS-DMA (global_load_lds_dwordx4: no VGPR staging, no ds_write pass) through an S-stage
// LDS ring: k-block kb + S - 1 is in flight while kb is multiplied, ordered by a counted vmcnt and a
// raw s_barrier per k-block (a __syncthreads would drain the DMA ring with vmcnt(0)). The DMA writes
// each wave-instruction's 1 KiB lane-linearly, so the bank-conflict swizzle is applied on the SOURCE
// side: 16-byte segment s of row r lands at segment s ^ f(r) (A8 / B: f = (r >> 2) & 3 over 64-byte
// rows; A16: f = (r >> 1) & 7 over 128-byte rows of raw int16 codes, split into hi / lo' on the
// fragment read), and the fragment reads apply the same XOR. Out-of-image taps and rows past M read a
// 16-byte fill block (0, or 0x80 for offset codes).
#include "igemm.h"
#include "pk2.h"

#include <type_traits>

namespace {

// waves per SIMD the register allocation must leave room for (4: two 512-thread workgroups per CU).
// 16-bit codes at BN 64: 142 -> 128 VGPRs (20 bytes of spill), two workgroups per CU: l1_c2 dgrad16
// 170.6 -> 155.6 us, the other shapes unchanged (profiles/r04l_ab probe_*.txt); A8 BN 128 at 3-4 stages
// would spill 200+ bytes. HALO int8 at BN 64: 98 VGPRs, two per CU. The pass-A epilogues (BNA) at BN 64
// fit 128 VGPRs (78 KiB of LDS: two workgroups per CU).
#ifndef LBT_BIG_OCC
#define LBT_BIG_OCC(A16, BN, S, HALO, BNA) \
  (((A16 && BN == 64 && !HALO && S <= 2) || (!A16 && HALO && BN == 64) || BNA == 4) ? 4 \
   : (A16 && BN == 64 && !HALO) ? 2 : 1)
#endif
// BN pass A (bn_wide.hip bn_bwd_a_wide_kernel) on the dgrad accumulators, element for element.
// MA = 1 (lbt_dgrad_bna): dx -> ReLU mask recomputed from R -> the BN's two quantisers. MA = 2, 3
// (lbt_dgrad_bn3): d = dx + g2 masked by y_bits (optionally stored) -> MA - 1 BNs' quantisers. Per BN:
// G2 = Q_rg(d) -> gamma-scaled rescale gradient -> G = Q_ng (stored) + the four channel sums + the
// counters. These launches tile the rows SAMPLE-blocked (igemm_big_kernel PERM): a 256-row x 64-column
// tile is 16 pixels x 16 samples. The dequantised dx tile is staged in LDS ([pixel][sample][column],
// padded: conflict-free writes from the MFMA layout and reads by quads), then pass A runs with
// bn_bwd_a_wide_kernel's thread layout: a thread owns one position (pixel, 4 channels) and walks 8
// samples, so its two Philox calls (or table reads) per BN are made once for 8 samples and a wave's
// loads / stores are 4 pixels x 64 contiguous channels of one sample (coalesced; the MFMA layout
// would touch 16 rows x 16 bytes per instruction). Channel sums: lanes of a quad column by shuffles,
// the 8 waves in LDS (int32: 16 samples x 16 pixels x 2^22), one int64 atomic per (BN, column, sum)
// into shard tile % NSHARD. Rows outside (sample >= N, pixel >= H*W) are skipped.
struct BnaBn {
  lbt_qdesc qrg, qng;
  const int8_t *R, *qn;
  const float* gamma;
  int16_t* gout;
  int64_t* sums;
};
template <int MA, int k>
LBT_DEV BnaBn bna_bn(const IgArgs& p) {
  if constexpr (MA == 1) {
    const lbt_dgrad_bna& b = p.bna;
    return BnaBn{b.qrg, b.qng, b.R, b.qn, b.gb, b.gout, b.sums};
  } else {
    const lbt_bna_bn& b = p.bn3.bn[k];
    return BnaBn{b.qrg, b.qng, b.R, b.qn, b.gamma_q, b.gout, b.sums};
  }
}
#ifndef LBT_EPI_UNROLL
#define LBT_EPI_UNROLL 8  // samples a thread of the staged epilogues has in flight (2: 1.1x slower, 4: spills; profiles/r04u)
#endif
constexpr int kXRow = 68;                // floats per (pixel, sample) row of the staged dx tile
constexpr int kXPix = 16 * kXRow + 4;    // floats per pixel: 16 samples + 4 (bank offset per pixel)
constexpr int kXBytes = 16 * kXPix * 4;  // 69 888 bytes

template <int MI, int NJ, int WM, int BN, int MA>
LBT_DEV void passa_epilogue(const IgArgs& p, const v4i (&acc)[2][MI][NJ], const v4i (&accw)[NJ], float scale,
                            int sb, int pb, int n0, int r, int q, int wm, uint32_t tile, int8_t* lds) {
  static_assert(BN == 64 && WM == 8 && MI == 2, "the pass-A epilogue runs 256 x 64 tiles of 8 waves");
  constexpr int NB = MA == 3 ? 2 : 1;
  const int C = p.ncol;
  const int N = p.d.N;
  const int hw = p.ch * p.cw;
  float* xs = reinterpret_cast<float*>(lds);
  // ---- the dequantised dx tile into LDS: lane (r, q) holds column 16 j + r of samples 4 q + e at pixel
  // MI wm + i
  __syncthreads();  // every wave's last fragment reads of the LDS ring are done
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int wsum = accw[j][0];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double hs = (double)acc[0][i][j][e] * 256.0;
        const double ls = (double)(acc[1][i][j][e] + 128 * wsum);
        xs[(wm * MI + i) * kXPix + (4 * q + e) * kXRow + j * 16 + r] = (float)(hs + ls) * scale;
      }
  }
  __syncthreads();
  // ---- pass A: thread = (quad cq, pixel pl, sample half sh)
  const int t = threadIdx.x;
  const int cq = t & 15, pl = (t >> 4) & 15, sh = t >> 8;
  const int c0 = n0 + 4 * cq;
  const int pix = pb * 16 + pl;
  const bool pv = pix < hw;
  float bet[4] = {0.f, 0.f, 0.f, 0.f};
  float sr = 0.f;
  if constexpr (MA == 1) {
    const float4 b4 = *reinterpret_cast<const float4*>(p.bna.gb + C + c0);
    bet[0] = b4.x; bet[1] = b4.y; bet[2] = b4.z; bet[3] = b4.w;
    sr = qstate(p.bna.qr).inv_m;
  }
  const uint64_t blk = ((uint64_t)(pv ? pix : 0) * (uint32_t)C + (uint32_t)c0) >> 2;
  const int sbase = sb * 16 + sh * 8;
  const int shard = (int)(tile % LBT_NSHARD);
  const int wv = t >> 6;
  int* red = reinterpret_cast<int*>(lds + kXBytes);  // [8 waves][4 sums][64 columns]
  // one pass over the thread's samples per BN (the projection blocks' two BNs one after the other: the
  // same registers)
  auto bn_pass = [&](auto kc) {
    constexpr int k = decltype(kc)::value;
    const BnaBn bn = bna_bn<MA, k>(p);
    const QState srg = qstate(bn.qrg), sng = qstate(bn.qng);
    const float4 g4 = *reinterpret_cast<const float4*>(bn.gamma + c0);
    const float gam[4] = {g4.x, g4.y, g4.z, g4.w};
    const Noise4 z{{0.f, 0.f, 0.f, 0.f}};
    const Noise4 u1 = bn.qrg.stochastic ? qnoise4(bn.qrg, srg.step, blk) : z;
    const Noise4 u2 = bn.qng.stochastic ? qnoise4(bn.qng, sng.step, blk) : z;
    int sm[4][4];  // [sum][channel]
#pragma unroll
    for (int a = 0; a < 4; ++a) sm[a][0] = sm[a][1] = sm[a][2] = sm[a][3] = 0;
    int ov[4] = {0, 0, 0, 0};
    // PK: both gradient quantisers stochastic (the models' configuration): quant4_w on packed pairs, the
    // counts as wave totals (lane 0 is active whenever a lane of its wave is: the inactive lanes of a sample
    // step are the wave's highest, past the image's last pixel); else quant1 per element, per-lane counts
    auto samples = [&](auto pkc) {
      constexpr bool PK = decltype(pkc)::value;
#pragma unroll LBT_EPI_UNROLL
      for (int u = 0; u < 8; ++u) {
        const int s_ = sbase + u;
        if (!pv || s_ >= N) break;  // samples ascend: the rest of this thread's are outside too
        const int64_t off = ((int64_t)s_ * hw + pix) * C + c0;
        const float4 xv = *reinterpret_cast<const float4*>(xs + pl * kXPix + (sh * 8 + u) * kXRow + 4 * cq);
        float d[4] = {xv.x, xv.y, xv.z, xv.w};
        const char4 rv = *reinterpret_cast<const char4*>(bn.R + off);
        const char4 qv = *reinterpret_cast<const char4*>(bn.qn + off);
        const int R[4] = {rv.x, rv.y, rv.z, rv.w};
        const int Q[4] = {qv.x, qv.y, qv.z, qv.w};
        if constexpr (MA >= 2) {  // bn_wide.hip :123-138
          const float4 g2 = *reinterpret_cast<const float4*>(p.bn3.g2 + off);
          const uint32_t yb = p.bn3.y_bits[off >> 2];
          d[0] = (yb & 1u) ? d[0] + g2.x : 0.f;
          d[1] = (yb & 2u) ? d[1] + g2.y : 0.f;
          d[2] = (yb & 4u) ? d[2] + g2.z : 0.f;
          d[3] = (yb & 8u) ? d[3] + g2.w : 0.f;
          if (k == 0 && p.bn3.gmask_out)
            *reinterpret_cast<float4*>(p.bn3.gmask_out + off) = make_float4(d[0], d[1], d[2], d[3]);
        } else {  // bn.hip chain_bwd_a's mask recomputation, op for op (bn_wide.hip :139-147)
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const float xr = (float)R[c] * sr;
            const float m1 = xr * gam[c];
            const float yv = m1 + bet[c];
            d[c] = yv > 0.f ? d[c] : 0.f;
          }
        }
        int G[4];
        if constexpr (PK) {  // bn_wide.hip :150-175 on packed pairs
          int G2[4];
          quant4_w<true>(srg, make_float4(d[0], d[1], d[2], d[3]), make_float4(u1.u[0], u1.u[1], u1.u[2], u1.u[3]), G2,
                         ov[0], ov[1]);
          const pf2 im = pk(srg.inv_m, srg.inv_m);
          const pf2 gh0 = pcvt(G2[0], G2[1]) * im, gh1 = pcvt(G2[2], G2[3]) * im;
          const pf2 dd0 = gh0 * pk(gam[0], gam[1]), dd1 = gh1 * pk(gam[2], gam[3]);
          quant4_w<true>(sng, make_float4(dd0.x, dd0.y, dd1.x, dd1.y), make_float4(u2.u[0], u2.u[1], u2.u[2], u2.u[3]),
                         G, ov[2], ov[3]);
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            sm[0][c] += G2[c] * R[c];
            sm[1][c] += G2[c];
            sm[2][c] += G[c];
            sm[3][c] += G[c] * Q[c];
          }
        } else {
#pragma unroll
          for (int c = 0; c < 4; ++c) {  // bn_wide.hip :150-175
            const int G2 = quant1(srg, bn.qrg.stochastic, d[c], u1.u[c], ov[0], ov[1]);
            sm[0][c] += G2 * R[c];
            sm[1][c] += G2;
            const float gh = (float)G2 * srg.inv_m;
            const float dd = gh * gam[c];
            G[c] = quant1(sng, bn.qng.stochastic, dd, u2.u[c], ov[2], ov[3]);
            sm[2][c] += G[c];
            sm[3][c] += G[c] * Q[c];
          }
        }
        short4 o;
        o.x = (short)G[0]; o.y = (short)G[1]; o.z = (short)G[2]; o.w = (short)G[3];
        *reinterpret_cast<short4*>(bn.gout + off) = o;
      }
    };
    const bool pkq = bn.qrg.stochastic && bn.qng.stochastic;  // uniform
    if (pkq)
      samples(std::true_type{});
    else
      samples(std::false_type{});
    // channel sums: the 4 pixel lanes of a wave sharing cq (shuffles), the 8 waves in LDS
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        int v = sm[a][c];
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        if ((t & 63) < 16) red[(wv * 4 + a) * 64 + 4 * cq + c] = v;
      }
    // overflow counts -> wave totals in lane 0 (already wave totals on the packed path)
    int a0 = ov[0], a1 = ov[1], b0 = ov[2], b1 = ov[3];
    if (!pkq) {
      a0 = wave_sum_i32(a0); a1 = wave_sum_i32(a1);
      b0 = wave_sum_i32(b0); b1 = wave_sum_i32(b1);
    }
    if ((t & 63) == 0) {
      if (bn.qrg.counts) {
        int32_t* ct = bn.qrg.counts + ((int64_t)bn.qrg.slot * LBT_NSHARD + shard) * LBT_CSTRIDE;
        if (a0) atomicAdd(ct, a0);
        if (a1) atomicAdd(ct + 1, a1);
      }
      if (bn.qng.counts) {
        int32_t* ct = bn.qng.counts + ((int64_t)bn.qng.slot * LBT_NSHARD + shard) * LBT_CSTRIDE;
        if (b0) atomicAdd(ct, b0);
        if (b1) atomicAdd(ct + 1, b1);
      }
    }
    __syncthreads();
    if (t < 256) {
      const int a = t >> 6, cl = t & 63;
      long long v = 0;
#pragma unroll
      for (int w = 0; w < 8; ++w) v += red[(w * 4 + a) * 64 + cl];
      if (v) atomicAdd((unsigned long long*)&bn.sums[(int64_t)shard * 4 * C + a * C + n0 + cl], (unsigned long long)v);
    }
    if (k + 1 < NB) __syncthreads();  // red is rewritten by the next BN's pass
  };
  bn_pass(std::integral_constant<int, 0>{});
  if constexpr (NB == 2) bn_pass(std::integral_constant<int, 1>{});
}

// The conv-output quantiser (Normalization_q's input, quant_epilogue's arithmetic) on sample-blocked
// tiles (BNA 4): per 64-column half, the dequantised tile is staged in LDS as for passa_epilogue, then a
// thread owns (pixel, 4 channels), draws that position's noise once (table or Philox) and walks 8
// samples -- int8 codes stored as coalesced char4 runs, exact channel sums (sum q, sum q^2) in
// registers, one int64 atomic per (column, sum) per workgroup (quant_epilogue: per column per wave).
template <int MI, int NJ, int WM, int BN>
LBT_DEV void quantq_epilogue(const IgArgs& p, const v4i (&acc)[MI][NJ], const v4i (&accw)[NJ], int u8, float scale,
                             int sb, int pb, int n0, int r, int q, int wm, int wn, uint32_t tile, int8_t* lds) {
  static_assert((BN == 64 && WM == 8 && MI == 2) || (BN == 128 && WM == 4 && MI == 4), "256 x 64 / 128 tiles");
  const int C = p.ncol;
  const int N = p.d.N;
  const int hw = p.ch * p.cw;
  const QState qs = qstate(p.qout);
  const int st = p.qout.stochastic;
  float* xs = reinterpret_cast<float*>(lds);
  int* red = reinterpret_cast<int*>(lds + kXBytes);  // [8 waves][2 sums][64 columns]
  const int t = threadIdx.x;
  const int cq = t & 15, pl = (t >> 4) & 15, sh = t >> 8, wv = t >> 6;
  const int pix = pb * 16 + pl;
  const bool pv = pix < hw;
  const int sbase = sb * 16 + sh * 8;
  const int shard = (int)(tile % LBT_NSHARD);
  int ov1 = 0, ov2 = 0;
  __syncthreads();  // every wave's last fragment reads of the LDS ring are done
#pragma unroll
  for (int h = 0; h < BN / 64; ++h) {
    if (wn == h) {  // this half's waves stage their rows: pixel MI wm + i, samples 4 q + e, column 16 j + r
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int wsum = accw[j][0];
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
          for (int e = 0; e < 4; ++e)
            xs[(wm * MI + i) * kXPix + (4 * q + e) * kXRow + j * 16 + r] = (float)(acc[i][j][e] + u8 * wsum) * scale;
      }
    }
    __syncthreads();
    const int c0 = n0 + h * 64 + 4 * cq;
    const uint64_t blk = ((uint64_t)(pv ? pix : 0) * (uint32_t)C + (uint32_t)c0) >> 2;
    Noise4 u = {{0.f, 0.f, 0.f, 0.f}};
    if (st) u = qnoise4(p.qout, qs.step, blk);
    const float4 u4 = make_float4(u.u[0], u.u[1], u.u[2], u.u[3]);
    int s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
    // this lane's samples sbase .. sbase + nsm - 1 (uniform per wave but for the pixel check): the
    // output pointer and the LDS row advance by one sample per step (no per-sample 64-bit offsets)
    const int nsm = pv ? (N - sbase < 8 ? (N - sbase > 0 ? N - sbase : 0) : 8) : 0;
    int8_t* yp = p.yq + ((int64_t)sbase * hw + pix) * C + c0;
    const int64_t ystep = (int64_t)hw * C;
    const float* xp = xs + pl * kXPix + (sh * 8) * kXRow + 4 * cq;
    auto samples = [&](auto stc) {
      constexpr bool ST = decltype(stc)::value;
#pragma unroll LBT_EPI_UNROLL
      for (int k = 0; k < 8; ++k) {
        if (k >= nsm) break;  // samples ascend
        const float4 xv = *reinterpret_cast<const float4*>(xp + k * kXRow);
        int c[4];
        quant4_w<ST>(qs, xv, u4, c, ov1, ov2);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          s1[e] += c[e];
          s2[e] += c[e] * c[e];
        }
        *reinterpret_cast<char4*>(yp) = make_char4((char)c[0], (char)c[1], (char)c[2], (char)c[3]);
        yp += ystep;
      }
    };
    if (st)
      samples(std::true_type{});
    else
      samples(std::false_type{});
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      int a = s1[e], b = s2[e];
      a += __shfl_xor(a, 16, 64);
      a += __shfl_xor(a, 32, 64);
      b += __shfl_xor(b, 16, 64);
      b += __shfl_xor(b, 32, 64);
      if ((t & 63) < 16) {
        red[(wv * 2 + 0) * 64 + 4 * cq + e] = a;
        red[(wv * 2 + 1) * 64 + 4 * cq + e] = b;
      }
    }
    __syncthreads();  // xs read and red written: the next half may restage
    if (t < 128) {
      const int a = t >> 6, cl = t & 63;
      long long v = 0;
#pragma unroll
      for (int w = 0; w < 8; ++w) v += red[(w * 2 + a) * 64 + cl];
      if (v)
        atomicAdd((unsigned long long*)&p.chsum[(int64_t)shard * 2 * C + a * C + n0 + h * 64 + cl], (unsigned long long)v);
    }
    if (h + 1 < BN / 64) __syncthreads();  // red is rewritten by the next half
  }
  // (wave totals, quant4_w: lane 0 was active whenever a lane of its wave was -- the inactive lanes of a
  // sample step are the ones past the image's last pixel, the wave's highest)
  if ((t & 63) == 0 && p.qout.counts) {
    int32_t* ct = p.qout.counts + ((int64_t)p.qout.slot * LBT_NSHARD + shard) * LBT_CSTRIDE;
    if (ov1) atomicAdd(ct, ov1);
    if (ov2) atomicAdd(ct + 1, ov2);
  }
}

// HALO (3x3, stride 1, pad 1: fwd, and the unit-stride dgrad of such a conv): the k loop runs
// channel-block-major, and per channel block ONE window of A is staged -- the tile's 256 pixels plus
// W + 1 on either side in the same row-major pixel order, 256 + 2W + 2 <= 384 rows -- instead of one
// 256-row A block per tap: the 9 taps read the window shifted by dy * W + dx (invalid taps -- outside
// the image -- read the fill value in registers). A leaves L2 ~1.4x instead of 9x per channel block.
// Window: two buffers, the next block's window DMA'd one instruction per wave per tap step while the
// current block's 9 taps run; B: a 3-stage ring, two taps ahead.
template <int MODE, bool A16, bool ADD, int BN, int S, int BNA = 0, bool HALO = false>
__global__ __launch_bounds__(kBT, LBT_BIG_OCC(A16, BN, S, HALO, BNA)) void igemm_big_kernel(IgArgs p) {
  constexpr int BM = 256, WN = BN / 64, WM = 8 / WN, TR = BM / WM, MI = TR / 16, NJ = 4;
  constexpr int NA = A16 ? 2 : 1;
  constexpr int ROWB = A16 ? 128 : 64;                 // bytes of one A row per k-block
  constexpr int ABYTES = BM * ROWB, BBYTES = BN * 64, STAGE = ABYTES + BBYTES;
  constexpr int NIA = ABYTES / 1024, NIB = BBYTES / 1024;  // 1-KiB DMA wave-instructions per stage
  constexpr int GA = NIA / 8;                          // A instructions per wave (2 or 4)
  constexpr int RPI = A16 ? 8 : 16;                    // A rows per instruction
  static_assert(NIA % 8 == 0 && (NIB % 8 == 0 || NIB == 4) && (!A16 || BN <= 128), "geometry");
  extern __shared__ __attribute__((aligned(16))) int8_t lds[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave / WN, wn = wave - wm * WN;
  const int r = lane & 15, q = lane >> 4;
  // XCD-aware bijective tile order: the WN column tiles of one row tile share an XCD's L2
  const int ntn = p.ncol / BN;
  const uint32_t nwg = gridDim.x, orig = blockIdx.x, xcd = orig % 8, qq = nwg / 8, rr = nwg % 8;
  const uint32_t tile = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + orig / 8;
  // PERM (the pass-A epilogues): row tile rt = (sample block sb, pixel block pb), tile row
  // (16 px + s) = pixel 16 pb + px of sample 16 sb + s; else rows m0 .. m0 + 255 in pixel order
  constexpr bool PERM = BNA >= 1;
  const uint32_t rt = tile / (uint32_t)ntn;
  const int64_t m0 = PERM ? 0 : (int64_t)rt * BM;
  const int sb = PERM ? (int)(rt / (uint32_t)p.npb) : 0, pb = PERM ? (int)(rt % (uint32_t)p.npb) : 0;
  const int n0 = (int)(tile % (uint32_t)ntn) * BN;
  const lbt_conv_desc& d = p.d;
  const int OH = p.ch, OW = p.cw;
  const int SH = MODE == MODE_FWD ? d.H : d.Ho, SW = MODE == MODE_FWD ? d.W : d.Wo;
  const int cblocks = p.cred / kBK, nk = p.nkh * p.nkw * cblocks;
  const int8_t* fill = (!A16 && p.a_u8off) ? reinterpret_cast<const int8_t*>(kFill80)
                                           : reinterpret_cast<const int8_t*>(zi());

  // ---- this lane's DMA rows: A row (i = wave + 8 g) * RPI + lane / (64 / RPI), segment lane % (64 / RPI)
  constexpr int SPR = 64 / RPI;  // lanes (16-byte segments) per row: 4 (A8) or 8 (A16)
  int an[GA], ay[GA], ax[GA], aseg[GA];
  bool arow[GA];
#pragma unroll
  for (int g = 0; g < GA; ++g) {
    const int row = (wave + 8 * g) * RPI + lane / SPR;
    if constexpr (PERM) {
      const int sm = sb * 16 + (row & 15), px = pb * 16 + (row >> 4);
      arow[g] = sm < d.N && px < OH * OW;
      const uint32_t pu = (uint32_t)(arow[g] ? px : 0);
      ax[g] = (int)(pu % (uint32_t)OW);
      ay[g] = (int)(pu / (uint32_t)OW);
      an[g] = arow[g] ? sm : 0;
    } else {
      const int64_t m = m0 + row;
      arow[g] = m < p.M;
      const uint32_t mu = (uint32_t)(arow[g] ? m : 0);
      ax[g] = (int)(mu % (uint32_t)OW);
      const uint32_t tt = mu / (uint32_t)OW;
      ay[g] = (int)(tt % (uint32_t)OH);
      an[g] = (int)(tt / (uint32_t)OH);
    }
    const int ps = lane % SPR;  // the LDS segment this lane fills; its source is segment ps ^ f(row)
    aseg[g] = A16 ? (ps ^ swz128(row)) : (ps ^ swz64(row));
  }
  // B: instruction i covers weight-image columns n0 + 16 i .. + 15 (64 bytes of the k-block each)
  constexpr int GB = NIB >= 8 ? NIB / 8 : 1;
  const bool bact = NIB >= 8 || wave < NIB;
  int bcolx[GB], bseg[GB];
#pragma unroll
  for (int g = 0; g < GB; ++g) {
    const int cl = (wave + 8 * g) * 16 + lane / 4;
    bcolx[g] = n0 + cl;
    bseg[g] = (lane % 4) ^ swz64(cl);
  }
  auto issue = [&](int kb, int st) {
    const int tap = kb / cblocks, cb = kb - tap * cblocks;
    const int th = tap / p.nkw, tw = tap - th * p.nkw;
    const int kh = MODE == MODE_FWD ? th : p.kh0 + d.SH * th, kw = MODE == MODE_FWD ? tw : p.kw0 + d.SW * tw;
    const int kbw = (kh * d.KW + kw) * cblocks + cb;
    int8_t* sb = lds + st * STAGE;
#pragma unroll
    for (int g = 0; g < GA; ++g) {
      int sy, sx;
      if (MODE == MODE_FWD) {
        sy = ay[g] * d.SH + kh - d.PT;
        sx = ax[g] * d.SW + kw - d.PL;
      } else {
        sy = ay[g] + p.oy - th;
        sx = ax[g] + p.ox - tw;
      }
      const bool ok = (unsigned)sy < (unsigned)SH && (unsigned)sx < (unsigned)SW && arow[g];
      const int8_t* src;
      if (ok) {
        const uint32_t pix = (uint32_t)((an[g] * SH + sy) * SW + sx);
        src = reinterpret_cast<const int8_t*>(p.a) +
              (uint64_t)(pix * (uint32_t)p.cred + (uint32_t)(cb * kBK)) * (A16 ? 2 : 1) + aseg[g] * 16;
      } else {
        src = fill;
      }
      __builtin_amdgcn_global_load_lds(src, (lds_vptr)(sb + (wave + 8 * g) * 1024), 16, 0, 0);
    }
    if (bact) {
#pragma unroll
      for (int g = 0; g < GB; ++g) {
        const int8_t* src = p.b + ((uint32_t)(bcolx[g] * p.ks + kbw * 4 + bseg[g]) << 4);
        __builtin_amdgcn_global_load_lds(src, (lds_vptr)(sb + ABYTES + (wave + 8 * g) * 1024), 16, 0, 0);
      }
    }
  };
  auto wait_landed = [&]() {  // k-block kb's DMA landed: at most S-2 younger groups in flight
    if constexpr (NIB >= 8) {
      vm_wait<(S - 2) * (GA + GB)>();
    } else {
      if (bact) vm_wait<(S - 2) * (GA + 1)>(); else vm_wait<(S - 2) * GA>();
    }
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
  // sum_k W per column (the +128 term of offset / split codes): from the caller's column sums when it
  // has them, else summed from the B fragments on the VALU (16-bit codes; offset codes of
  // lbt_conv_fwd_igemm_q) -- 4 v_dot4 per fragment instead of an MFMA against ones (an extra 4 of
  // the 16 (A8) / 32 (A16) MFMAs per k-block of a 64 x 64 wave tile)
  const bool wmfma = A16 || (p.a_u8off && !p.colsum);  // uniform
  int csw[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) csw[j] = 0;

  // fragments of one k-block (A16: the raw int16 code pairs, split into hi / lo' at the MFMA)
  typedef v4i FragA[MI][NA];
  typedef v4i FragB[NJ];
  auto read_frags = [&](int st, FragA& fa, FragB& fb) {
    const int8_t* sb = lds + st * STAGE;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int col = wn * 64 + j * 16 + r;
      fb[j] = *reinterpret_cast<const v4i*>(sb + ABYTES + col * 64 + ((q ^ swz64(col)) << 4));
    }
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int row = wm * TR + i * 16 + r;
      if constexpr (A16) {
        const int f = swz128(row);
        fa[i][0] = *reinterpret_cast<const v4i*>(sb + row * 128 + (((2 * q) ^ f) << 4));
        fa[i][NA - 1] = *reinterpret_cast<const v4i*>(sb + row * 128 + (((2 * q + 1) ^ f) << 4));
      } else {
        fa[i][0] = *reinterpret_cast<const v4i*>(sb + row * 64 + ((q ^ swz64(row)) << 4));
      }
    }
  };
  auto mma = [&](const FragA& fa, const FragB& fb) {
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      if constexpr (A16) {
        // codes (int16) e0 e1 | e2 e3 per dword: hi = high bytes, lo' = low bytes ^ 0x80 (a = 256 hi + lo' + 128)
        const v4i c0 = fa[i][0], c1 = fa[i][NA - 1];
        const uint32_t w[8] = {(uint32_t)c0[0], (uint32_t)c0[1], (uint32_t)c0[2], (uint32_t)c0[3],
                               (uint32_t)c1[0], (uint32_t)c1[1], (uint32_t)c1[2], (uint32_t)c1[3]};
        v4i hi, lo;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          hi[u] = (int)__builtin_amdgcn_perm(w[2 * u + 1], w[2 * u], 0x07050301u);
          lo[u] = (int)(__builtin_amdgcn_perm(w[2 * u + 1], w[2 * u], 0x06040200u) ^ 0x80808080u);
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          acc[0][i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(hi, fb[j], acc[0][i][j], 0, 0, 0);
          acc[NA - 1][i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(lo, fb[j], acc[NA - 1][i][j], 0, 0, 0);
        }
      } else {
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          acc[0][i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[i][0], fb[j], acc[0][i][j], 0, 0, 0);
      }
    }
    if (wmfma) {  // sum_k W of the column: the lane's 16 k-bytes on the VALU (dot4 with ones), beside the MFMAs
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int u = 0; u < 4; ++u) csw[j] = __builtin_amdgcn_sdot4(fb[j][u], 0x01010101, csw[j], false);
    }
  };

  if constexpr (HALO) {
    constexpr int GW = A16 ? 6 : 3;        // window DMA instructions per wave: 8 * GW * RPI = 384 rows
    constexpr int NWR = 8 * GW * RPI, WINB = NWR * ROWB, BST = BN * 64;
    constexpr int GBI = NIB >= 8 ? NIB / 8 : 1;  // B instructions per issuing wave per tap
    int8_t* win = lds;                     // [2][NWR][ROWB]
    int8_t* bring = lds + 2 * WINB;        // [3][BN][64]
    const int Wd = OW, Hd = OH;
    const int nwin = 256 + 2 * Wd + 2;     // window rows that can be read
    const int64_t wbase = m0 - (Wd + 1);
    uint32_t soff[GW];
    bool sv[GW];
#pragma unroll
    for (int g = 0; g < GW; ++g) {
      const int wr = (wave + 8 * g) * RPI + lane / SPR;
      const int64_t px = wbase + wr;
      sv[g] = wr < nwin && px >= 0 && px < p.M;
      const int ps = lane % SPR;
      const int sg = A16 ? (ps ^ swz128(wr)) : (ps ^ swz64(wr));
      soff[g] = sv[g] ? (uint32_t)px * (uint32_t)p.cred * (A16 ? 2u : 1u) + (uint32_t)sg * 16u : 0u;
    }
    auto issue_win = [&](int cb, int buf, int g) {
      const int8_t* src = sv[g] ? reinterpret_cast<const int8_t*>(p.a) + soff[g] + (uint32_t)cb * (A16 ? 128u : 64u)
                                : fill;
      __builtin_amdgcn_global_load_lds(src, (lds_vptr)(win + buf * WINB + (wave + 8 * g) * 1024), 16, 0, 0);
    };
    auto issue_b = [&](int k, int st) {
      const int cb = k / 9, tp = k - cb * 9;
      const int kbw = tp * cblocks + cb;  // (kh * 3 + kw) * cblocks + cb
      if (bact) {
#pragma unroll
        for (int g = 0; g < GB; ++g) {
          const int8_t* src = p.b + ((uint32_t)(bcolx[g] * p.ks + kbw * 4 + bseg[g]) << 4);
          __builtin_amdgcn_global_load_lds(src, (lds_vptr)(bring + st * BST + (wave + 8 * g) * 1024), 16, 0, 0);
        }
      }
    };
    // this lane's fragment rows: pixel (x, y) within its image, and whether the row exists
    int fx[MI], fy[MI];
    bool fok[MI];
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int64_t m = m0 + wm * TR + i * 16 + r;
      fok[i] = m < p.M;
      const uint32_t mu = (uint32_t)(fok[i] ? m : 0);
      fx[i] = (int)(mu % (uint32_t)Wd);
      fy[i] = (int)((mu / (uint32_t)Wd) % (uint32_t)Hd);
    }
    const int afill = (!A16 && p.a_u8off) ? (int)0x80808080u : 0;
#pragma unroll
    for (int g = 0; g < GW; ++g) issue_win(0, 0, g);
    issue_b(0, 0);
    issue_b(nk > 1 ? 1 : 0, 1);
    for (int cb = 0; cb < cblocks; ++cb) {
      const bool more = cb + 1 < cblocks;
      const int8_t* wsb = win + (cb & 1) * WINB;
      auto tap_step = [&](auto tc) {
        constexpr int tp = decltype(tc)::value;
        constexpr int th = tp / 3, tw = tp % 3;
        constexpr int dy = MODE == MODE_FWD ? th - 1 : 1 - th, dx = MODE == MODE_FWD ? tw - 1 : 1 - tw;
        // B(k) landed: younger are B(k + 1) and the window pieces of steps k - 2, k - 1
        constexpr int P = (tp >= 2 && tp - 2 < GW ? 1 : 0) + (tp >= 1 && tp - 1 < GW ? 1 : 0);
        if (bact) {
          if (more) vm_wait<GBI + P>(); else vm_wait<GBI>();
        } else {
          if (more) vm_wait<P>(); else vm_wait<0>();
        }
        __builtin_amdgcn_s_barrier();
        const int k = cb * 9 + tp;
        issue_b(k + 2 < nk ? k + 2 : nk - 1, (tp + 2) % 3);
        if (tp < GW && more) issue_win(cb + 1, (cb + 1) & 1, tp);
        FragA fa;
        FragB fb;
        const int8_t* bsb = bring + (tp % 3) * BST;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const int col = wn * 64 + j * 16 + r;
          fb[j] = *reinterpret_cast<const v4i*>(bsb + col * 64 + ((q ^ swz64(col)) << 4));
        }
#pragma unroll
        for (int i = 0; i < MI; ++i) {
          const int wr = wm * TR + i * 16 + r + (dy + 1) * Wd + dx + 1;
          const bool v = fok[i] && (unsigned)(fx[i] + dx) < (unsigned)Wd && (unsigned)(fy[i] + dy) < (unsigned)Hd;
          if constexpr (A16) {
            const int f = swz128(wr);
            const v4i c0 = *reinterpret_cast<const v4i*>(wsb + wr * 128 + (((2 * q) ^ f) << 4));
            const v4i c1 = *reinterpret_cast<const v4i*>(wsb + wr * 128 + (((2 * q + 1) ^ f) << 4));
            const v4i z = v4i{0, 0, 0, 0};
            fa[i][0] = v ? c0 : z;
            fa[i][NA - 1] = v ? c1 : z;
          } else {
            const v4i c0 = *reinterpret_cast<const v4i*>(wsb + wr * 64 + ((q ^ swz64(wr)) << 4));
            fa[i][0] = v ? c0 : v4i{afill, afill, afill, afill};
          }
        }
        mma(fa, fb);
      };
      tap_step(std::integral_constant<int, 0>{});
      tap_step(std::integral_constant<int, 1>{});
      tap_step(std::integral_constant<int, 2>{});
      tap_step(std::integral_constant<int, 3>{});
      tap_step(std::integral_constant<int, 4>{});
      tap_step(std::integral_constant<int, 5>{});
      tap_step(std::integral_constant<int, 6>{});
      tap_step(std::integral_constant<int, 7>{});
      tap_step(std::integral_constant<int, 8>{});
    }
  } else {
#pragma unroll
  for (int s = 0; s < S - 1; ++s) issue(s < nk ? s : nk - 1, s);
  if constexpr (S >= 3) {
    // Software-pipelined: k-block kb + 1's fragments are read from LDS while kb's MFMAs run. Step kb
    // waits for DMA group kb + 1 (at most S - 3 younger groups in flight) and the barrier, which also
    // retires every wave's reads of the stage the new DMA (group kb + S - 1) overwrites (read in step kb - 2).
    auto wait_next = [&]() {
      if constexpr (NIB >= 8) {
        vm_wait<(S - 3) * (GA + GB)>();
      } else {
        if (bact) vm_wait<(S - 3) * (GA + 1)>(); else vm_wait<(S - 3) * GA>();
      }
    };
    auto step = [&](int kb, const FragA& ca, const FragB& cb, FragA& na, FragB& nb) {
      wait_next();
      __builtin_amdgcn_s_barrier();
      if (!(p.dbg & 1)) {
        const int nx = kb + S - 1;
        issue(nx < nk ? nx : nk - 1, nx % S);
      }
      read_frags((kb + 1) % S, na, nb);  // past the last k-block: an unused read of a stale stage
      mma(ca, cb);
    };
    wait_landed();
    __builtin_amdgcn_s_barrier();
    FragA fa0, fa1;
    FragB fb0, fb1;
    read_frags(0, fa0, fb0);
    for (int kb = 0; kb < nk; kb += 2) {
      step(kb, fa0, fb0, fa1, fb1);
      if (kb + 1 < nk) step(kb + 1, fa1, fb1, fa0, fb0);
    }
  } else {
    for (int kb = 0; kb < nk; ++kb) {
      wait_landed();
      __builtin_amdgcn_s_barrier();
      if (!(p.dbg & 1)) {
        const int nx = kb + S - 1;
        issue(nx < nk ? nx : nk - 1, nx % S);  // refills the stage read in iteration kb - 1
      }
      FragA fa;
      FragB fb;
      read_frags(kb % S, fa, fb);
      mma(fa, fb);
    }
  }
  }
  vm_wait<0>();  // the ring's trailing (clamped) DMAs: nothing may still write LDS when the block ends
  if (wmfma) {  // the column totals: lanes r, r + 16, r + 32, r + 48 hold a quarter of column r's k each
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const auto h = __builtin_amdgcn_permlane32_swap(csw[j], csw[j], false, false);
      const int t1 = (int)h[0] + (int)h[1];
      const auto g = __builtin_amdgcn_permlane16_swap(t1, t1, false, false);
      const int t = (int)g[0] + (int)g[1];
      accw[j] = v4i{t, t, t, t};
    }
  }

  // ---- epilogue (igemm_kernel's): lane owns column (tile col + r), rows (tile row + 4q + e)
  const float scale = ldexpf(1.0f, -(frac_exp(p.qa) + frac_exp(p.qb)));
  constexpr bool addv = MODE == MODE_DGRAD && ADD;
  const int ncol = p.ncol;
  const int64_t rtile = m0 + wm * TR + q * 4;  // + i * 16 + e
  const bool full = m0 + BM <= p.M;
  const int rlim = full ? TR : (int)(p.M - rtile);
  const int cw = n0 + wn * 64;
  // the +128 sum_k W term of offset codes: the weight image's column sums (fwd); 16-bit codes: accw
  if constexpr (!A16) {
    if (p.a_u8off && p.colsum) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int cs = p.colsum[cw + j * 16 + r];
        accw[j] = v4i{cs, cs, cs, cs};
      }
    }
  }
  const int u8 = (!A16 && p.a_u8off) ? 128 : 0;
  if constexpr (BNA == 4) {
    if constexpr (MODE == MODE_FWD && !A16)
      quantq_epilogue<MI, NJ, WM, BN>(p, acc[0], accw, u8, scale, sb, pb, n0, r, q, wm, wn, tile, lds);
    return;
  }
  if constexpr (MODE == MODE_FWD && !A16) {
    if (p.yq) {  // uniform: quantising epilogue
      quant_epilogue<MI, NJ>(p, acc[0], accw, u8, scale, rtile, rlim, full, cw, r, q);
      return;
    }
  }
  if constexpr (BNA >= 1 && BNA <= 3) {
    if constexpr (BN == 64) passa_epilogue<MI, NJ, WM, BN, BNA>(p, acc, accw, scale, sb, pb, n0, r, q, wm, tile, lds);
    return;
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int col = cw + j * 16 + r;
    float* yp = p.y + rtile * ncol + col;
    const float* ap = addv ? p.add_src + rtile * ncol + col : nullptr;
    float av[MI][4];
    if constexpr (addv) {
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) av[i][e] = (i * 16 + e < rlim) ? ap[(i * 16 + e) * ncol] : 0.f;
    }
    const int wsum = (A16 || p.a_u8off) ? accw[j][0] : 0;
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v;
        if constexpr (A16) {
          const double hs = (double)acc[0][i][j][e] * 256.0;
          const double ls = (double)(acc[1][i][j][e] + 128 * wsum);
          v = (float)(hs + ls) * scale;
        } else {
          v = (float)(acc[0][i][j][e] + u8 * wsum) * scale;
        }
        if (full || i * 16 + e < rlim) yp[(i * 16 + e) * ncol] = addv ? v + av[i][e] : v;
      }
  }
}

// one igemm_big_kernel instantiation: dynamic LDS = the S-stage ring, or (HALO) two A windows of 384
// rows + a 3-stage B ring
template <int MODE, bool A16, bool ADD, int BN, int S, int BNA, bool HALO>
void big_go(const IgArgs& p, int64_t tiles, hipStream_t st) {
  constexpr int BM = 256, ROWB = A16 ? 128 : 64;
  constexpr size_t ring = HALO ? (size_t)2 * 384 * ROWB + (size_t)3 * BN * 64 : (size_t)S * (BM * ROWB + BN * 64);
  // the staged dx tile + the channel-sum exchange of the pass-A epilogue
  constexpr size_t shm = (BNA && ring < (size_t)kXBytes + 8192) ? (size_t)kXBytes + 8192 : ring;
  launch_dyn_lds<&igemm_big_kernel<MODE, A16, ADD, BN, S, BNA, HALO>>(dim3((unsigned)tiles), dim3(kBT), shm, st, p);
}

template <int MODE, bool A16, int BN, int S, bool HALO = false>
void launch_big_bn(IgArgs p, hipStream_t st) {
  static const int dbg = getenv_int("LBT_IGEMM_BIG_DBG", 0);
  p.dbg = dbg;
  // sample-blocked tiles only for the instantiations that decode them (the kernel's PERM)
  const bool qperm = MODE == MODE_FWD && !A16 && BN <= 128 && S == 2 && !HALO && p.perm && p.yq;
  const bool bna = MODE == MODE_DGRAD && A16 && BN == 64 && !HALO && p.has_bna;
  if (!qperm && !bna) p.perm = 0;
  const int64_t rtiles = p.perm ? (int64_t)((p.d.N + 15) / 16) * p.npb : (p.M + 255) / 256;
  const int64_t tiles = rtiles * (p.ncol / BN);
  if constexpr (MODE == MODE_DGRAD && A16 && BN == 64 && !HALO) {
    if (p.has_bna == 1) return big_go<MODE, A16, false, BN, S, 1, HALO>(p, tiles, st);
    if (p.has_bna == 2 && p.bn3.nbn == 1) return big_go<MODE, A16, false, BN, S, 2, HALO>(p, tiles, st);
    if (p.has_bna == 2) return big_go<MODE, A16, false, BN, S, 3, HALO>(p, tiles, st);
  }
  if constexpr (MODE == MODE_FWD && !A16 && BN <= 128 && S == 2 && !HALO) {
    if (qperm) return big_go<MODE, A16, false, BN, S, 4, HALO>(p, tiles, st);
  }
  if (MODE == MODE_DGRAD && p.add_src) big_go<MODE, A16, MODE == MODE_DGRAD, BN, S, 0, HALO>(p, tiles, st);
  else big_go<MODE, A16, false, BN, S, 0, HALO>(p, tiles, st);
}

// Selection of the 256-row LDS-DMA kernel (lbt_igemm_tuning, include/lbt_dfxp.h): read per call,
// so a test can force the kernel onto any shape and variant. Defaults from the environment at the
// first use (LBT_IGEMM_BIG, LBT_IGEMM_BIG_MIN, LBT_IGEMM_BIG_S, LBT_IGEMM_BIG_BN256) -- the measured
// choice: on, >= 200 tiles, 2 stages, 128-column tiles at most.
lbt_igemm_tuning& big_tuning() {
  static lbt_igemm_tuning t = [] {
    lbt_igemm_tuning v;
    v.big = getenv_int("LBT_IGEMM_BIG", 1);
    v.min_tiles = getenv_int("LBT_IGEMM_BIG_MIN", 200);
    v.stages = getenv_int("LBT_IGEMM_BIG_S", 2);
    v.max_bn = getenv_int("LBT_IGEMM_BIG_BN256", 0) ? 256 : 128;
    v.halo = getenv_int("LBT_IGEMM_HALO", 1);  // bit 0: int8 codes (fwd), bit 1: 16-bit codes (dgrad16)
    v.fwdq_perm = getenv_int("LBT_FWDQ_PERM", 2);
    v.launches = 0;
    return v;
  }();
  return t;
}

// The 256-row LDS-DMA kernel takes a GEMM when it is big enough to give every CU about one tile
// (min_tiles, default 200; big = 0: never) and is not split / classed.
template <int MODE, bool A16>
bool launch_big(const IgArgs& p, hipStream_t st) {
  const lbt_igemm_tuning tu = big_tuning();
  const int64_t tmin = tu.min_tiles;
  if (!tu.big || p.ksplit != 1 || p.ncol % 64 || p.cred % kBK) return false;
  if ((p.M + 255) / 256 * (p.ncol / 64) > 0x7fffffff) return false;
  // column tile: the widest (<= max_bn) that still gives min_tiles tiles (256 only without the
  // quantising epilogue and on request: its 8 x 4 accumulator tiles per wave spill)
  const int64_t mt = p.perm ? (int64_t)((p.d.N + 15) / 16) * p.npb : (p.M + 255) / 256;
  int bn = 0;
  if (!A16 && !p.yq && p.ncol % 256 == 0 && tu.max_bn >= 256 && mt * (p.ncol / 256) >= tmin) bn = 256;
  else if (tu.max_bn >= 128 && p.ncol % 128 == 0 && mt * (p.ncol / 128) >= tmin) bn = 128;
  else if (mt * (p.ncol / 64) >= tmin) bn = 64;
  if (!bn) return false;
  if (p.has_bna) bn = 64;  // the pass-A epilogues: 64-column tiles, 256 VGPRs (one workgroup per CU)
  // LDS ring depth (stages): 2 by default -- the probe on the ResNet-50 shapes measured the
  // occupancy of 2 stages (A8 BN 128: 48 KiB, two workgroups per CU) ahead of the latency hiding of 3-4
  // (72-96 KiB, one; the software-pipelined loop), except 3x3 dgrad16 at 28x28 / 14x14 (3-5 %).
  // A16 runs 3 stages for any request above 2 (4 stages of 128-byte A rows at BN 128 would take 160 KiB).
  const int S = tu.stages;
  // 3x3 / stride 1 / pad 1 with every tap (fwd, unit-stride dgrad) and W <= 63: the A window per
  // channel block (HALO), 64- and 128-column tiles
  const lbt_conv_desc& d = p.d;
  const bool halo = (tu.halo & (A16 ? 2 : 1)) && !p.perm && bn <= 128 && d.KH == 3 && d.KW == 3 && d.SH == 1 && d.SW == 1 && d.PT == 1 &&
                    d.PL == 1 && d.Ho == d.H && d.Wo == d.W && p.nkh == 3 && p.nkw == 3 && p.kh0 == 0 &&
                    p.kw0 == 0 && p.cw == d.W && p.ch == d.H && d.W <= 63 &&
                    // where it measured faster (profiles/r04p): one column tile (the window is not
                    // re-staged per column tile), or a chip the 128-column tiles would under-fill
                    (p.ncol == 64 || mt * (p.ncol / bn) < 256);
  if constexpr (MODE == MODE_DGRAD && A16) {
    if (p.has_bna == 1 && p.perm >= 2 && igemm_launch_dgrada_persist(p, st)) {
      ++big_tuning().launches;
      return true;
    }
  }
  if constexpr (MODE == MODE_FWD && !A16) {
    if (p.yq && p.perm >= 2 && bn <= 128 && igemm_launch_fwdq_persist(bn, p, S, st)) {
      ++big_tuning().launches;
      return true;
    }
  }
  if (halo) {  // 64-column tiles: int8 codes two workgroups per CU (98 VGPRs, 60 KiB); 16-bit one (2 x 48 KiB windows)
    launch_big_bn<MODE, A16, 64, 2, true>(p, st);
  } else if (bn == 256) {
    if constexpr (!A16) launch_big_bn<MODE, A16, 256, 4>(p, st);
  } else if (bn == 128) {
    if (S <= 2) launch_big_bn<MODE, A16, 128, 2>(p, st);
    else if (S == 3 || A16) launch_big_bn<MODE, A16, 128, 3>(p, st);
    else launch_big_bn<MODE, A16, 128, 4>(p, st);
  } else {
    if (S <= 2) launch_big_bn<MODE, A16, 64, 2>(p, st);
    else if (S == 3) launch_big_bn<MODE, A16, 64, 3>(p, st);
    else launch_big_bn<MODE, A16, 64, 4>(p, st);
  }
  ++big_tuning().launches;
  return true;
}

}  // namespace

bool lbt::igemm_launch_big(int mode, bool a16, const IgArgs& p, hipStream_t st) {
  if (mode == MODE_FWD) return a16 ? launch_big<MODE_FWD, true>(p, st) : launch_big<MODE_FWD, false>(p, st);
  return a16 ? launch_big<MODE_DGRAD, true>(p, st) : launch_big<MODE_DGRAD, false>(p, st);
}

int lbt::igemm_fwdq_perm() { return big_tuning().fwdq_perm; }

// lbt_igemm_tuning: the 256-row kernel's selection, read by every wide fwd / dgrad call after this
extern "C" int lbt_igemm_get_tuning(lbt_igemm_tuning* out) {
  if (!out) return LBT_EINVAL;
  *out = big_tuning();
  return 0;
}

extern "C" int lbt_igemm_set_tuning(const lbt_igemm_tuning* t) {
  if (!t || t->min_tiles < 1 || t->stages < 2 || t->stages > 4 || (t->max_bn != 64 && t->max_bn != 128 && t->max_bn != 256) ||
      t->fwdq_perm < 0 || t->fwdq_perm > 4096)
    return LBT_EINVAL;
  lbt_igemm_tuning& cur = big_tuning();
  cur.big = t->big; cur.min_tiles = t->min_tiles; cur.stages = t->stages; cur.max_bn = t->max_bn;
  cur.halo = t->halo;
  cur.fwdq_perm = t->fwdq_perm;
  return 0;
}
